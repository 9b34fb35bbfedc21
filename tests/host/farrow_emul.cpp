// Host emulation of the Farrow resampler's index algebra (no GPU): csrc/farrow_core.hpp's n_old and mu, computed with the
// reciprocal-and-remainder division the kernel uses, must be bit-identical to the reference's plain IEEE divisions
//     n_old = floor(j*Ts_new / Ts_old),  mu = (j*Ts_new - n_old*Ts_old) / Ts_old
// over 10^7 output indices per ratio (the first 4 M in a row, the rest random up to 2^31), integer ratios included.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I scikit-dsp-comm_amd/csrc tests/host/farrow_emul.cpp -o /tmp/farrow_emul
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include "farrow_core.hpp"

using namespace skdsp::farrow;

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    const double kPi = 3.14159265358979311600, kE = 2.71828182845904509080;
    const double ratios[][2] = {{8, 18}, {48000, 44100}, {1, kPi}, {kE, 1}, {15, 14}, {3, 3}, {1, 1}, {7, 7},
                                {10, 9.999}, {44100, 48000}, {1e6, 1}, {1, 1000}, {96000, 44100}, {kPi, kE}};
    std::mt19937_64 g(2024);
    long long bad = 0, total = 0;
    for (const auto &fs : ratios) {
        const volatile double fo = fs[0], fn = fs[1];
        const double ts_old = 1.0 / fo, ts_new = 1.0 / fn, r = 1.0 / ts_old;
        std::uniform_int_distribution<int64_t> pick(0, ((int64_t)1 << 31) - 1);
        long long bad_here = 0;
        for (int64_t i = 0; i < 10000000; ++i) {
            const int64_t j = i < 4000000 ? i : pick(g);
            const double t = (double)j * ts_new;
            const volatile double tv = t, tso = ts_old;
            const double n_ref = std::floor(tv / tso);
            const double mu_ref = (t - n_ref * ts_old) / tso;
            const Index ix = index_of((double)j, ts_old, ts_new, r);
            if (!same(ix.n_old, n_ref) || !same(ix.mu, mu_ref)) {
                if (bad_here < 5)
                    std::printf("mismatch fs %.17g -> %.17g  j=%lld  n_old %.17g / %.17g  mu %.17g / %.17g\n", (double)fo, (double)fn,
                                (long long)j, ix.n_old, n_ref, ix.mu, mu_ref);
                ++bad_here;
            }
        }
        std::printf("fs %.10g -> %.10g: %lld mismatches in 10^7 indices\n", (double)fo, (double)fn, bad_here);
        bad += bad_here;
        total += 10000000;
    }
    // the output count against a direct count of the arange's elements (start + i*step < stop for i < len)
    long long bad_len = 0;
    for (int64_t n : {0, 1, 2, 3, 4, 5, 17, 1000, 123457}) {
        for (const auto &fs : ratios) {
            const double ts_old = 1.0 / fs[0], ts_new = 1.0 / fs[1];
            const int64_t len = out_len(n, ts_old, ts_new);
            const double stop = ts_old * (double)(n - 3) + ts_old;
            int64_t direct = 0;
            while ((double)direct * ts_new < stop) ++direct;   // len = ceil(stop/step); i*step < stop is the same test up to rounding
            if (len < 0 || (len != direct && std::fabs((double)(len - direct)) > 1)) ++bad_len;
        }
    }
    std::printf("%lld mismatches in %lld indices, %lld length outliers\n", bad, total, bad_len);
    if (bad == 0 && bad_len == 0) std::printf("OK\n");
    return bad == 0 && bad_len == 0 ? 0 : 1;
}
