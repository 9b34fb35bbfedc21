// Host emulation of the Welch primitive on float32 samples (no GPU): csrc/psd_core.hpp's in-place FFT passes over a float64
// or a float32 image, computed in float64 between load and store, and its |X|^2 accumulation, run thread by thread and pass by pass
// exactly as csrc/psd.hip schedules them (real input: two segments per complex transform, folded at the end), with the
// twiddles and the window in float64.
//   psd_emul n_fft ns step nseg is_real x.f32 window.f64 out.f64 image_bits      (image_bits: 32 or 64, the LDS image psd.hip keeps)
// x.f32: float32 samples (interleaved re, im unless is_real); out.f64: S[0 .. n_fft) as float64.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I scikit-dsp-comm_amd/csrc tests/host/psd_emul.cpp -o /tmp/psd_emul
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "psd_core.hpp"

using namespace skdsp::psd;

static std::vector<float> g_x;
static std::vector<double> g_w;
static int g_ns, g_step, g_real;
static long long g_nseg;

template <typename T, int LOG2N> static void run(std::vector<double> &S)
{
    typedef Core<T, double, LOG2N> C;
    const int N = C::N;
    const double kTwoPi = 6.283185307179586476925286766559;
    std::vector<cx<double>> tw(N);
    std::vector<cx<T>> img(N);
    for (int i = 0; i < N; ++i) tw[i] = cx<double>{std::cos(kTwoPi * i / N), -std::sin(kTwoPi * i / N)};
    std::vector<double> acc((size_t)C::TS * C::NACC, 0.0), P(N, 0.0);
    const int pack = g_real ? 2 : 1;
    for (long long seg = 0; seg < g_nseg; seg += pack) {
        const bool second = g_real && seg + 1 < g_nseg;
        auto ld = [&](int n) {
            if (n >= g_ns) return cx<double>{0., 0.};
            const long long i = seg * g_step + n;
            if (g_real) return cx<double>{g_x[i] * g_w[n], second ? g_x[i + g_step] * g_w[n] : 0.};
            return cx<double>{g_x[2 * i] * g_w[n], g_x[2 * i + 1] * g_w[n]};
        };
        for (int t = 0; t < C::TS; ++t) C::first(t, ld, tw.data(), img.data());
        for (int s = 1; s < C::NSTORE; ++s)
            for (int t = 0; t < C::TS; ++t) C::mid(s, t, tw.data(), img.data());
        for (int t = 0; t < C::TS; ++t) C::last(t, img.data(), &acc[(size_t)t * C::NACC]);
    }
    for (int t = 0; t < C::TS; ++t)
        for (int i = 0; i < C::R; ++i)
            for (int m = 0; m < 4; ++m) P[C::bin_of(4 * (t + C::TS * i) + m)] = acc[(size_t)t * C::NACC + 4 * i + m];
    S.resize(N);
    for (int f = 0; f < N; ++f) S[f] = g_real ? 0.5 * (P[f] + P[(N - f) % N]) : P[f];
}

int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    const bool img64 = std::atoi(argv[9]) == 64;
    const int n_fft = std::atoi(argv[1]);
    g_ns = std::atoi(argv[2]);
    g_step = std::atoi(argv[3]);
    g_nseg = std::atoll(argv[4]);
    g_real = std::atoi(argv[5]);
    const size_t need = (size_t)((g_nseg - 1) * g_step + g_ns) * (g_real ? 1 : 2);
    g_x.resize(need);
    FILE *f = std::fopen(argv[6], "rb");
    if (!f || std::fread(g_x.data(), 4, need, f) != need) return 3;
    std::fclose(f);
    std::vector<double> w(g_ns);
    f = std::fopen(argv[7], "rb");
    if (!f || std::fread(w.data(), 8, g_ns, f) != (size_t)g_ns) return 4;
    std::fclose(f);
    g_w.assign(w.begin(), w.end());
    std::vector<double> S;
    switch (n_fft) {
    case 64: img64 ? run<double, 6>(S) : run<float, 6>(S); break;
    case 128: img64 ? run<double, 7>(S) : run<float, 7>(S); break;
    case 256: img64 ? run<double, 8>(S) : run<float, 8>(S); break;
    case 512: img64 ? run<double, 9>(S) : run<float, 9>(S); break;
    case 1024: img64 ? run<double, 10>(S) : run<float, 10>(S); break;
    case 2048: img64 ? run<double, 11>(S) : run<float, 11>(S); break;
    case 4096: img64 ? run<double, 12>(S) : run<float, 12>(S); break;
    default: return 5;
    }
    f = std::fopen(argv[8], "wb");
    if (!f || std::fwrite(S.data(), 8, S.size(), f) != S.size()) return 6;
    std::fclose(f);
    std::printf("OK\n");
    return 0;
}
