// Host run of the V32 admission model (no GPU): csrc/iir_par_plan.hpp's par_v32_input_error -- the float32 chain of the matrix instruction, bit for bit --
// on the designs of tests/golden/g18_v32_designs.npz and on inputs the probe itself does not run.  For every design the library admits at a chunk
// length, the worst state-error share must leave room for the rest of the kernel inside the 1e-6 contract: kParV32Limit's promise, checked.
// Build: g++ -O2 -std=c++17 -pthread -I scikit-dsp-comm_amd/csrc tests/host/iir_par_v32_emul.cpp -o /tmp/iir_par_v32_emul
// Run:   iir_par_v32_emul designs.txt           the check (exit status 1 where an admitted design exceeds the bound)
//        iir_par_v32_emul --rank designs.txt    per design and T the three detuned frequencies the model ranks worst (tests/golden/gen_golden_v32.py)
// designs.txt:  "design NAME NSEC", NSEC rows "b0 b1 b2 a0 a1 a2", then any number of "worst T f f f" rows (the stored frequencies)
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "iir_par_plan.hpp"

using namespace skdsp;

struct Design {
    std::string name;
    int nsec = 0;
    double coef[40] = {};
    std::vector<double> worst[2];   // [0]: T = 128, [1]: T = 96
};

static bool read_designs(const char *path, std::vector<Design> &out)
{
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char word[64], name[128];
    bool ok = true;
    while (ok && std::fscanf(f, "%63s", word) == 1) {
        if (!std::strcmp(word, "design")) {
            Design d;
            ok = std::fscanf(f, "%127s %d", name, &d.nsec) == 2 && d.nsec >= 1 && d.nsec <= 8;
            d.name = name;
            for (int k = 0; ok && k < d.nsec; ++k) {
                double r[6];
                for (int i = 0; i < 6; ++i) ok = ok && std::fscanf(f, "%lf", &r[i]) == 1;
                if (!ok || r[3] == 0.0) { ok = false; break; }
                const double c[5] = {r[0] / r[3], r[1] / r[3], r[2] / r[3], r[4] / r[3], r[5] / r[3]};
                std::memcpy(d.coef + 5 * k, c, sizeof c);
            }
            if (ok) out.push_back(d);
        } else if (!std::strcmp(word, "worst") && !out.empty()) {
            int T = 0;
            double v[3];
            ok = std::fscanf(f, "%d %lf %lf %lf", &T, &v[0], &v[1], &v[2]) == 4 && (T == 128 || T == 96);
            if (ok) out.back().worst[T == 128 ? 0 : 1].assign(v, v + 3);
        } else
            ok = false;
    }
    std::fclose(f);
    return ok && !out.empty();
}

static const int kGridChunks = 96, kLongChunks = 512;   // (the GPU test runs 384 chunks of 128 and 512 of 96)
static const double kGridStep = 0.001;
static const int kGridHalf = 30;                         // +- 0.03 rad / sample

struct Model {
    const ParExpansion &P;
    ParV32G G;
    std::vector<float> x;
    Model(const ParExpansion &p, int T) : P(p), G(par_v32_g(p, T)), x((size_t)kLongChunks * T) {}
    template <typename F> double run(int nch, F &&sample)
    {
        const int n = nch * G.T;
        for (int i = 0; i < n; ++i) x[(size_t)i] = (float)sample(i);
        return par_v32_input_error(P, G, x.data(), nch);
    }
    double tone(double w, int nch) { return run(nch, [&](int i) { return std::cos(w * i); }); }
};

// the detune grid around every resonance: (error, frequency), worst first
static std::vector<std::pair<double, double>> detune_grid(Model &m)
{
    std::vector<std::pair<double, double>> r;
    for (int k = 0; k < m.P.nsec; ++k) {
        const double th = par_resonance(m.P, k);
        if (th < 0.0) continue;
        for (int g = -kGridHalf; g <= kGridHalf; ++g) {
            const double w = th + kGridStep * g;
            if (w <= 0.0 || w >= 3.141592653589793) continue;
            r.emplace_back(m.tone(w, kGridChunks), w);
        }
    }
    std::sort(r.begin(), r.end(), [](const std::pair<double, double> &a, const std::pair<double, double> &b) { return a.first > b.first; });
    return r;
}

struct Result {
    std::string text;
    bool failed = false, admitted = false;
};

static std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// one design at one chunk length: the ranking of the detune grid, or the check
static Result run_one(const Design &d, int ti, bool rank, double bound)
{
    Result res;
    ParExpansion P;
    if (!par_expand(d.coef, d.nsec, P)) {
        res.text = fmt("%s: the parallel form refuses this cascade\n", d.name.c_str());
        res.failed = true;
        return res;
    }
    const int T = ti == 0 ? 128 : 96;
    Model m(P, T);
    if (rank) {
        const auto g = detune_grid(m);
        res.text = fmt("worst %s %d", d.name.c_str(), T);
        for (size_t i = 0; i < 3; ++i) res.text += fmt(" %.17g", i < g.size() ? g[i].second : 0.0);
        res.text += "\n";
        return res;
    }
    const double probe = par_v32_probe(P, T);
    res.admitted = probe <= kParV32Limit;
    struct Row { const char *what; double e; };
    std::vector<Row> rows;
    rows.push_back({"probe", probe});
    double e_sin = 0.0, e_snap = 0.0, e_long = 0.0, e_up[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < P.nsec; ++k) {
        const double th = par_resonance(P, k);
        if (th < 0.0) continue;
        e_sin = std::max(e_sin, m.run(kGridChunks, [&](int i) { return std::sin(th * i); }));
        e_long = std::max(e_long, std::max(m.tone(th, kLongChunks), m.run(kLongChunks, [&](int i) { return std::sin(th * i); })));
        const double step = 2.0 * 3.141592653589793 / T;
        e_snap = std::max(e_snap, m.tone(std::round(th / step) * step, kGridChunks));
        for (int L = 2; L <= 4; ++L)   // a low-rate tone cos(L th j) zero-stuffed by L and scaled by L: one of its images sits on the resonance
            e_up[L - 2] = std::max(e_up[L - 2], m.run(kGridChunks, [&](int i) { return i % L ? 0.0 : L * std::cos(th * i); }));
    }
    rows.push_back({"resonance sine", e_sin});
    rows.push_back({"resonance, 512 chunks", e_long});
    const auto g = detune_grid(m);
    rows.push_back({"detune grid", g.empty() ? 0.0 : g[0].first});
    rows.push_back({"resonance snapped to 2 pi / T", e_snap});
    rows.push_back({"square wave of period T", m.run(kGridChunks, [&](int i) { return i % T < T / 2 ? 1.0 : -1.0; })});
    rows.push_back({"comb of period T", std::max(m.run(kGridChunks, [&](int i) { return i % T == 0 ? 1.0 : 0.0; }),
                                                 m.run(kGridChunks, [&](int i) { return i % T == T - 1 ? 1.0 : 0.0; }))});
    rows.push_back({"zero-stuffed by 2", e_up[0]});
    rows.push_back({"zero-stuffed by 3", e_up[1]});
    rows.push_back({"zero-stuffed by 4", e_up[2]});
    double e_stored = 0.0;
    for (double w : d.worst[ti]) e_stored = std::max(e_stored, m.tone(w, kLongChunks));
    rows.push_back({"stored worst tones, 512 chunks", e_stored});
    double worst = 0.0;
    const char *where = "";
    for (const Row &r : rows)
        if (!(r.e <= worst)) { worst = r.e; where = r.what; }
    res.text = fmt("%-30s T = %3d  probe %.3e (%a) %s  worst %.3e (%s), %.2f of the probe", d.name.c_str(), T, probe, probe,
                   res.admitted ? "admitted" : "refused ", worst, where, worst / probe);
    if (res.admitted && !(worst < bound)) {
        res.text += fmt("  FAILED: above %.3e", bound);
        res.failed = true;
    }
    res.text += "\n";
    for (const Row &r : rows) res.text += fmt("    %-34s %.3e\n", r.what, r.e);
    return res;
}

int main(int argc, char **argv)
{
    const bool rank = argc == 3 && !std::strcmp(argv[1], "--rank");
    std::vector<Design> designs;
    if ((argc != 2 && !rank) || !read_designs(argv[argc - 1], designs)) {
        std::printf("usage: iir_par_v32_emul [--rank] designs.txt\n");
        return 2;
    }
    const double bound = 1e-6 - kParV32Rest;
    // (design, chunk length) pairs are independent: a few threads share them
    std::vector<Result> results(designs.size() * 2);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t j; (j = next++) < results.size();) results[j] = run_one(designs[j / 2], (int)(j % 2), rank, bound);
    };
    std::vector<std::thread> pool;
    const unsigned nthr = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    for (unsigned i = 1; i < nthr; ++i) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    int failed = 0, admitted_n[2] = {0, 0};
    for (size_t j = 0; j < results.size(); ++j) {
        std::fputs(results[j].text.c_str(), stdout);
        failed += results[j].failed;
        admitted_n[j % 2] += results[j].admitted;
    }
    if (rank) return failed ? 1 : 0;
    std::printf("admitted: %d of %zu at T = 128, %d at T = 96; bound %.3e = 1e-6 - %.1e\n", admitted_n[0], designs.size(), admitted_n[1], bound, kParV32Rest);
    if (failed) {
        std::printf("%d check(s) failed\n", failed);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
