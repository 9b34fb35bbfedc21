// Host emulation of the Viterbi kernel (no GPU): csrc/viterbi_core.hpp's trellis, lane mapping, distances and per-state step, walked
// lane by lane and slot by slot exactly as csrc/viterbi.hip schedules them: 64 lanes, states per lane and predecessor lanes / slots from
// the core's mapping (K <= 7: one state per lane, 64 / Ns streams per wave of which stream `group` is walked here; K = 8, 9: lane l holds
// states l + 64 slot), int32 metrics with the step's minimum subtracted for hard / soft, float64 for unquant, the first lane attaining the
// minimum found slot by slot.
//   viterbi_emul polys depth metric quant_level group out.u8 in1.f64 [in2.f64 ...]
// polys: G1,G2[,G3]; metric 0 / 1 / 2 (hard / soft / unquant); inN.f64: the received values of call N as float64 (soft: int() is taken here);
// the calls run on ONE decoder state; out.u8: the decided bits of all calls, one byte each, concatenated.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I scikit-dsp-comm_amd/csrc tests/host/viterbi_emul.cpp -o /tmp/viterbi_emul
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "viterbi_core.hpp"

using namespace skdsp::vit;

template <int METRIC, int W> struct Wave {
    typedef typename Dist<METRIC>::MT MT;
    Plan p;
    int base;   // first lane of the walked stream
    std::vector<MT> M;            // [lane][slot]
    std::vector<uint32_t> H;      // [lane][slot][W]
    Wave(const Plan &plan, int group) : p(plan), base(group * lanes_of(plan.K)), M((size_t)kWave * plan.spl, MT(0)), H((size_t)kWave * plan.spl * W, 0u) {}
    MT &m(int lane, int slot) { return M[(size_t)lane * p.spl + slot]; }
    uint32_t *h(int lane, int slot) { return &H[((size_t)lane * p.spl + slot) * W]; }

    // one symbol; returns the decided bit
    unsigned step(const MT *v, int top)
    {
        const int GL = lanes_of(p.K), NP = p.spl > 1 ? p.spl / 2 : 1;
        MT d[3][2];
        Dist<METRIC>::both(v, p.R, top, d);
        std::vector<MT> Mn(M);
        std::vector<uint32_t> Hn(H);
        for (int lane = base; lane < base + GL; ++lane) {
            const int pl = pred_lane(lane, p.Ns);
            for (int jj = 0; jj < NP; ++jj) {
                const int ps = pred_slot(lane, jj, p.Ns);
                for (int half = 0; half < (p.spl > 1 ? 2 : 1); ++half) {
                    const int j = jj + half * NP, s = state_of(lane, j, p.Ns), p0 = pred0(s, p.Ns);
                    const unsigned u = in_bit(s, p.K);
                    if (state_of(pl, ps, p.Ns) != p0 || state_of(pl + 1, ps, p.Ns) != p0 + 1) {
                        fprintf(stderr, "lane mapping: state %d expects predecessors %d, %d\n", s, p0, p0 + 1);
                        exit(3);
                    }
                    acs<MT, W>(m(pl, ps), m(pl + 1, ps), branch_metric<MT>(d, p.R, branch_word(p.gmask, p.R, p.K, p0, u)),
                               branch_metric<MT>(d, p.R, branch_word(p.gmask, p.R, p.K, p0 + 1, u)), h(pl, ps), h(pl + 1, ps), u,
                               &Mn[(size_t)lane * p.spl + j], &Hn[((size_t)lane * p.spl + j) * W]);
                }
            }
        }
        M.swap(Mn);
        H.swap(Hn);
        MT mn = m(base, 0);
        for (int lane = base; lane < base + GL; ++lane)
            for (int j = 0; j < p.spl; ++j) mn = m(lane, j) < mn ? m(lane, j) : mn;
        unsigned bit = 0;
        bool found = false;
        for (int j = 0; j < p.spl && !found; ++j)
            for (int lane = base; lane < base + GL && !found; ++lane)
                if (m(lane, j) == mn) {
                    bit = oldest_bit(h(lane, j), p.depth);
                    found = true;
                }
        if (METRIC != kUnquant)
            for (int lane = base; lane < base + GL; ++lane)
                for (int j = 0; j < p.spl; ++j) m(lane, j) -= mn;
        return bit;
    }
};

static std::vector<double> read_f64(const char *path)
{
    std::vector<double> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(4);
    double b[256];
    size_t n;
    while ((n = fread(b, sizeof(double), 256, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}

template <int METRIC, int W> static int run(const Plan &p, int quant, int group, const char *outp, int nin, char **in)
{
    typedef typename Dist<METRIC>::MT MT;
    Wave<METRIC, W> wave(p, group);
    std::vector<unsigned char> out;
    for (int c = 0; c < nin; ++c) {
        const std::vector<double> x = read_f64(in[c]);
        const int64_t nsym = symbols_of(p, (int64_t)x.size());
        for (int64_t t = 0; t < nsym; ++t) {
            MT v[3] = {MT(0), MT(0), MT(0)};
            for (int k = 0; k < p.R; ++k) {
                const size_t i = (size_t)t * p.R + k;
                if (METRIC == kHard) v[k] = i < x.size() ? (MT)x[i] : (MT)kAbsent;
                else if (METRIC == kSoft) v[k] = (MT)(long long)x[i];   // toward zero
                else v[k] = (MT)x[i];
            }
            const unsigned bit = wave.step(v, (1 << quant) - 1);
            if (t >= p.depth - 1) out.push_back((unsigned char)bit);
        }
    }
    FILE *f = fopen(outp, "wb");
    if (!f) return 4;
    if (!out.empty()) fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    std::string polys = argv[1];
    std::vector<std::string> g;
    size_t at = 0;
    while (true) {
        const size_t c = polys.find(',', at);
        g.push_back(polys.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    const char *ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < g.size() && i < 4; ++i) ptr[i] = g[i].c_str();
    Plan p;
    const char *why = plan_make(ptr, (int)g.size(), std::atoi(argv[2]), &p);
    if (why) {
        fprintf(stderr, "%s\n", why);
        return 5;
    }
    const int metric = std::atoi(argv[3]), quant = std::atoi(argv[4]), group = std::atoi(argv[5]);
    if (group < 0 || group >= p.streams) return 6;
    const int nin = argc - 7;
#define RUN(MET) (p.words == 2 ? run<MET, 2>(p, quant, group, argv[6], nin, argv + 7) : run<MET, 4>(p, quant, group, argv[6], nin, argv + 7))
    return metric == kHard ? RUN(kHard) : metric == kSoft ? RUN(kSoft) : RUN(kUnquant);
}
