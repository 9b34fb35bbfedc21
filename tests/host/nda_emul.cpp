// nda_emul.cpp -- the symbol timing kernels of csrc/timing.hip walked thread by thread on the CPU from csrc/timing_core.hpp: the same plans, index algebra and
// arithmetic, with every global access checked against the windows the call owns and every LDS access checked against the image (and against reading a
// word no lane has written).  A stand-alone program: tests/test_nda_cpu.py builds it plain and with -fsanitize=address,undefined and runs it as a child
// process.
//
//   nda_emul plan <ns> <L>               lanes, tile iterations, samples of a tile's row, LDS row pitch, LDS doubles, threads of the scale kernel
//   nda_emul iters <n> <ns>              the loop's iterations for a frame of n samples
//   nda_emul rows <dtype> <ns> <L> <iord> <outputs> <normalize> <n> <nrow> <start> <x_stride> <y_stride> <cap> <k1> <k2> <per_row> <inv_ns> <inv_len> <k_eps>
//                 <gains.bin> <rot.bin> <x.bin> <out prefix>
//                                        gains.bin: nrow pairs (read if per_row); rot.bin: ns real parts, then ns imaginary parts;
//                                        writes <prefix>z.bin, e.bin for the selected outputs and <prefix>c.bin, the counts
// x.bin holds exactly the elements from the first row's first to the last row's last that the call may read; the buffers are allocated to that size, so a
// sanitizer sees one element too many.  Output blocks are filled with the byte 0xA5 before the walk: what lies behind a row's count, and the gaps between
// the rows, must come back as they were.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "timing_core.hpp"

using namespace skdsp;

static void die(const char *what)
{
    fprintf(stderr, "nda_emul: %s\n", what);
    exit(2);
}

struct Range {
    const char *lo, *hi;
};
struct CheckedMem {
    std::vector<Range> rd, wr;
    void check(const std::vector<Range> &rs, const void *p, size_t bytes, const char *what) const
    {
        const char *c = static_cast<const char *>(p);
        for (const Range &r : rs)
            if (c >= r.lo && c + bytes <= r.hi) return;
        die(what);
    }
    double ld_f64(const double *g) const
    {
        check(rd, g, 8, "global read outside the call's windows");
        return *g;
    }
    uint64_t ld_u64(const void *g) const
    {
        check(rd, g, 8, "global read outside the call's windows");
        uint64_t v;
        memcpy(&v, g, 8);
        return v;
    }
    void ld_c128(const double *g, double *re, double *im) const
    {
        check(rd, g, 16, "global read outside the call's windows");
        *re = g[0];
        *im = g[1];
    }
    void st_f64(double *g, double v) const
    {
        check(wr, g, 8, "global write outside the rows");
        *g = v;
    }
    void st_c64(float *g, float re, float im) const
    {
        check(wr, g, 8, "global write outside the rows");
        g[0] = re;
        g[1] = im;
    }
    void st_c128(double *g, double re, double im) const
    {
        check(wr, g, 16, "global write outside the rows");
        g[0] = re;
        g[1] = im;
    }
};

struct CheckedLds {
    double *w;
    unsigned char *written;
    int size;
    double ld(int i) const
    {
        if (i < 0 || i >= size) die("LDS read outside the image");
        if (!written[i]) die("LDS read of a word nobody wrote");
        return w[i];
    }
    void ld2(int i, double *a, double *b) const
    {
        if (i & 1) die("misaligned 16-byte LDS read");
        *a = ld(i);
        *b = ld(i + 1);
    }
    void st(int i, double v) const
    {
        if (i < 0 || i >= size) die("LDS write outside the image");
        w[i] = v;
        written[i] = 1;
    }
    void st2(int i, double a, double b) const
    {
        if (i & 1) die("misaligned 16-byte LDS write");
        st(i, a);
        st(i + 1, b);
    }
};

static std::vector<char> read_file(const char *path, size_t want)
{
    std::vector<char> v(want ? want : 1);
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open an input file");
    if (want && fread(v.data(), 1, want, f) != want) die("short input file");
    fclose(f);
    v.resize(want);
    v.shrink_to_fit();
    return v;
}
static void write_file(const std::string &path, const void *p, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) die("cannot write the output file");
    fclose(f);
}

template <bool C64> static void fetch_all(const CheckedMem &m, const tim::Plan &p, const void *x, int64_t group, int64_t tile, std::vector<car::Sample> &regs)
{
    for (int t = 0; t < tim::kLane; ++t) tim::tile_fetch<C64>(m, p, x, group, tile, t, &regs[(size_t)t * tim::kMaxW]);
}
template <class... A> static void walk_ord(int iord, A &&...a)
{
    if (iord == 1)
        tim::tile_walk<1>(a...);
    else if (iord == 2)
        tim::tile_walk<2>(a...);
    else
        tim::tile_walk<3>(a...);
}

// nda_norm_kernel, phase by phase
static void run_norm(const CheckedMem &m, const tim::NormPlan &np, const double *raw, void *y, const int64_t *counts)
{
    const int T = tim::kNormThreads;
    std::vector<double> slots(2 * T);
    std::vector<unsigned char> written(2 * T);
    const CheckedLds S = {slots.data(), written.data(), 2 * T};
    for (int64_t row = 0; row < np.nrow; ++row) {
        const int64_t n = tim::norm_len(m, np, counts, row);
        if (n == 0) continue;
        std::fill(written.begin(), written.end(), 0);
        for (int t = 0; t < T; ++t) tim::norm_sums(m, np, raw, row, n, t, S);
        for (int off = T / 2; off >= 1; off >>= 1)
            for (int t = 0; t < T; ++t) tim::norm_tree(off, t, S);
        double sr, si;
        S.ld2(0, &sr, &si);
        const double mr = sr / (double)n, mi = si / (double)n;
        for (int t = 0; t < T; ++t) tim::norm_dists(m, np, raw, row, n, t, mr, mi, S);
        for (int off = T / 2; off >= 1; off >>= 1)
            for (int t = 0; t < T; ++t) tim::norm_tree(off, t, S);
        double q, unused;
        S.ld2(0, &q, &unused);
        const double rcp = 1.0 / sqrt(q / (double)n);
        for (int t = 0; t < T; ++t) tim::norm_store(m, np, raw, y, row, n, t, rcp);
    }
}

static int run_rows(char **v)
{
    const int dtype = atoi(v[0]), ns = atoi(v[1]), L = atoi(v[2]), iord = atoi(v[3]), outs = atoi(v[4]), normalize = atoi(v[5]);
    const int64_t n = atoll(v[6]), nrow = atoll(v[7]), start = atoll(v[8]), x_stride = atoll(v[9]), y_stride = atoll(v[10]), cap = atoll(v[11]);
    const double k1 = strtod(v[12], nullptr), k2 = strtod(v[13], nullptr);
    const int per_row = atoi(v[14]);
    const bool want_z = (outs & tim::kOutZ) != 0, want_e = (outs & tim::kOutE) != 0;
    const bool norm = want_z && normalize && cap > 0, via_scratch = norm && dtype == 1;
    tim::Plan p;
    if (const char *why = tim::plan_make(ns, L, iord, dtype, dtype == 1 && !via_scratch, outs, n, nrow, start, x_stride, y_stride, cap, &p)) die(why);
    if (via_scratch) p.z_stride = cap;
    const int esz = dtype == 1 ? 8 : 16;
    const bool any = nrow > 0;
    std::vector<char> gains = read_file(v[18], per_row ? (size_t)nrow * 16 : 0), rot = read_file(v[19], (size_t)ns * 16);
    std::vector<char> x = read_file(v[20], any && n > 0 ? (size_t)((nrow - 1) * x_stride + start + n) * esz : 0);
    const size_t rows = any && cap > 0 ? (size_t)((nrow - 1) * y_stride + cap) : 0;
    std::vector<char> z(want_z ? rows * esz : 0, (char)0xA5), e(want_e ? rows * 8 : 0, (char)0xA5), counts(any ? (size_t)nrow * 8 : 0, (char)0xA5);
    std::vector<char> scratch(via_scratch ? (size_t)nrow * cap * 16 : 0, (char)0xA5);
    CheckedMem m;
    m.rd.push_back({gains.data(), gains.data() + gains.size()});
    m.wr.push_back({counts.data(), counts.data() + counts.size()});
    for (int64_t row = 0; any && row < nrow; ++row) {
        if (n > 0) m.rd.push_back({x.data() + (row * x_stride + start) * esz, x.data() + (row * x_stride + start + n) * esz});
        if (want_z && cap > 0) m.wr.push_back({z.data() + row * y_stride * esz, z.data() + (row * y_stride + cap) * esz});
        if (want_e && cap > 0) m.wr.push_back({e.data() + row * y_stride * 8, e.data() + (row * y_stride + cap) * 8});
    }
    if (via_scratch) m.wr.push_back({scratch.data(), scratch.data() + scratch.size()});
    std::vector<double> rr(tim::kMaxNs), ri(tim::kMaxNs);
    for (int i = 0; i < ns; ++i) {
        memcpy(&rr[i], rot.data() + 8 * i, 8);
        memcpy(&ri[i], rot.data() + 8 * (ns + i), 8);
    }
    tim::Loop lp;
    lp.ns = ns;
    lp.len = 2 * L + 1;
    lp.inv_ns = strtod(v[15], nullptr);
    lp.inv_len = strtod(v[16], nullptr);
    lp.k_eps = strtod(v[17], nullptr);
    lp.rot_re = rr.data();
    lp.rot_im = ri.data();
    std::vector<double> image((size_t)p.lds_doubles);
    std::vector<unsigned char> written((size_t)p.lds_doubles);
    const CheckedLds Lds = {image.data(), written.data(), p.lds_doubles};
    const double *gp = per_row ? reinterpret_cast<const double *>(gains.data()) : nullptr;
    void *zp = via_scratch ? (void *)scratch.data() : (void *)z.data();
    double *ep = reinterpret_cast<double *>(e.data());
    int64_t *cp = reinterpret_cast<int64_t *>(counts.data());
    for (int64_t group = 0; any && group < p.groups; ++group) {
        tim::Row w[tim::kLane];
        tim::State st[tim::kLane];
        std::vector<car::Sample> regs((size_t)tim::kLane * tim::kMaxW);
        std::fill(written.begin(), written.end(), 0);
        for (int t = 0; t < tim::kLane; ++t) {
            w[t] = tim::row_of(m, k1, k2, gp, group * tim::kLane + t, nrow);
            st[t] = tim::state_rest();
            tim::ring_clear(p, t, Lds);
        }
        if (p.tiles > 0) p.c64 ? fetch_all<true>(m, p, x.data(), group, 0, regs) : fetch_all<false>(m, p, x.data(), group, 0, regs);
        for (int64_t tile = 0; tile < p.tiles; ++tile) {
            std::fill(written.begin(), written.begin() + p.at_ring, 0);
            for (int t = 0; t < tim::kLane; ++t)
                p.c64 ? tim::tile_put<true>(p, t, &regs[(size_t)t * tim::kMaxW], Lds) : tim::tile_put<false>(p, t, &regs[(size_t)t * tim::kMaxW], Lds);
            if (tile + 1 < p.tiles) p.c64 ? fetch_all<true>(m, p, x.data(), group, tile + 1, regs) : fetch_all<false>(m, p, x.data(), group, tile + 1, regs);
            for (int t = 0; t < tim::kLane; ++t) walk_ord(iord, m, p, lp, w[t], group, tile, t, st[t], Lds, zp, ep);
        }
        for (int t = 0; t < tim::kLane; ++t) {
            const int64_t row = group * tim::kLane + t;
            if (row < nrow) {
                m.check(m.wr, cp + row, 8, "global write outside the counts");
                cp[row] = st[t].mm - 1;
            }
        }
    }
    if (norm && any) {
        tim::NormPlan np;
        if (const char *why = tim::norm_plan_make(dtype == 1, nrow, cap, via_scratch ? cap : y_stride, y_stride, &np)) die(why);
        CheckedMem m2;
        m2.rd.push_back({counts.data(), counts.data() + counts.size()});
        const std::vector<char> &src = via_scratch ? scratch : z;
        const int64_t rs = via_scratch ? cap : y_stride;
        for (int64_t row = 0; row < nrow; ++row) {
            m2.rd.push_back({src.data() + row * rs * 16, src.data() + (row * rs + cap) * 16});
            m2.wr.push_back({z.data() + row * y_stride * esz, z.data() + (row * y_stride + cap) * esz});
        }
        run_norm(m2, np, reinterpret_cast<const double *>(src.data()), z.data(), cp);
    }
    const std::string prefix = v[21];
    if (want_z) write_file(prefix + "z.bin", z.data(), z.size());
    if (want_e) write_file(prefix + "e.bin", e.data(), e.size());
    write_file(prefix + "c.bin", counts.data(), counts.size());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "plan" && argc == 4) {
        tim::Plan p;
        if (const char *why = tim::plan_make(atoi(argv[2]), atoi(argv[3]), 3, 3, 0, 3, 0, 1, 0, 0, 0, 0, &p)) die(why);
        printf("%d %d %d %d %d %d\n", tim::kLane, tim::kTile, p.W, p.pitch, p.lds_doubles, tim::kNormThreads);
        return 0;
    }
    if (cmd == "iters" && argc == 4) {
        printf("%lld\n", (long long)tim::loop_iters(atoll(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (cmd == "rows" && argc == 24) return run_rows(argv + 2);
    die("usage: plan <ns> <L> | iters <n> <ns> | rows ...");
    return 2;
}
