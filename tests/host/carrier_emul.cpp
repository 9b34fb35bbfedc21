// carrier_emul.cpp -- the carrier loop kernel and the impairment kernel of csrc/carrier.hip walked thread by thread on the CPU from csrc/carrier_core.hpp: the
// same plans, index algebra and arithmetic, with every global access checked against the windows the call owns and every LDS access checked against the
// image (and against reading a word no lane has written in this tile).  A stand-alone program: tests/test_carrier_cpu.py builds it plain and with
// -fsanitize=address,undefined and runs it as a child process.
//
//   carrier_emul plan                    lanes, tile symbols, LDS row pitch
//   carrier_emul lds <outputs>           LDS doubles of a launch that produces the outputs of the mask
//   carrier_emul funcs <n> <in.bin> <out.bin>
//                                        in: n pairs (a, b) of doubles; out: n rows (sin a, cos a, wrap_2pi(a), atan2_rn(a, b), sign_np(a), cdiv_imag_np(a, b, b, a))
//   carrier_emul rows <dtype> <fam> <mod> <type> <open_loop> <outputs> <n> <nrow> <start> <step> <x_stride> <y_stride> <k1> <k2> <per_row> <inv_sqrt2>
//                     <gains.bin> <r.bin> <tab.bin> <x.bin> <out prefix>
//                                        gains.bin: nrow pairs (read if per_row); r.bin: nrow doubles (QAM); tab.bin: mod (re, im) pairs (MPSK above 4);
//                                        writes <prefix>z.bin, a.bin, e.bin, t.bin for the selected outputs
//   carrier_emul imp <mode> <dtype> <n> <n_out> <nrow> <ns> <n_step> <x_stride> <y_stride> <shift> <per_row> <c> <d> <vals.bin> <x.bin> <y.bin>
//                                        vals.bin: nrow int64 shifts (mode 0) or nrow (c, d) pairs (mode 1), read if per_row
// x.bin holds exactly the elements from the first row's first to the last row's last that the call may read; the buffers are allocated to that size, so a
// sanitizer sees one element too many.  Output blocks are filled with the byte 0xA5 before the walk: the gaps between the rows must come back as they were.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "carrier_core.hpp"

using namespace skdsp;

static void die(const char *what)
{
    fprintf(stderr, "carrier_emul: %s\n", what);
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
    void ld_c64(const float *g, double *re, double *im) const
    {
        check(rd, g, 8, "global read outside the call's windows");
        *re = (double)g[0];
        *im = (double)g[1];
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

template <int FAM> static void walk_type(int type, const car::Plan &p, const car::Loop &lp, const car::Row &w, int64_t group, int64_t tile, int t, car::State &st, const CheckedLds &L)
{
    if (type == 0)
        car::tile_walk<FAM, 0>(p, lp, w, group, tile, t, st, L);
    else if (type == 1)
        car::tile_walk<FAM, 1>(p, lp, w, group, tile, t, st, L);
    else
        car::tile_walk<FAM, 2>(p, lp, w, group, tile, t, st, L);
}

template <bool C64> static void fetch_all(const CheckedMem &m, const car::Plan &p, const void *x, int64_t group, int64_t tile, std::vector<car::Sample> &regs)
{
    for (int t = 0; t < car::kLane; ++t) car::tile_fetch<C64>(m, p, x, group, tile, t, &regs[(size_t)t * car::kPer]);
}

static int run_rows(char **v)
{
    const int dtype = atoi(v[0]), fam = atoi(v[1]), mod = atoi(v[2]), type = atoi(v[3]), open_loop = atoi(v[4]), outs = atoi(v[5]);
    const int64_t n = atoll(v[6]), nrow = atoll(v[7]), start = atoll(v[8]), step = atoll(v[9]), x_stride = atoll(v[10]), y_stride = atoll(v[11]);
    const double k1 = strtod(v[12], nullptr), k2 = strtod(v[13], nullptr), inv_sqrt2 = strtod(v[15], nullptr);
    const int per_row = atoi(v[14]);
    car::Plan p;
    if (const char *why = car::plan_make(fam, mod, type, dtype, outs, n, nrow, start, step, x_stride, y_stride, &p)) die(why);
    const int esz = dtype == 1 ? 8 : 16;
    const bool any = n > 0 && nrow > 0;
    const int64_t span = any ? start + (n - 1) * step + 1 : 0;
    std::vector<char> gains = read_file(v[16], per_row ? (size_t)nrow * 16 : 0), r = read_file(v[17], fam == sym::kQam ? (size_t)nrow * 8 : 0);
    std::vector<char> tab = read_file(v[18], (fam == sym::kMpsk && mod > 4) ? (size_t)mod * 16 : 0);
    std::vector<char> x = read_file(v[19], any ? (size_t)((nrow - 1) * x_stride + span) * esz : 0);
    const size_t rows = any ? (size_t)((nrow - 1) * y_stride + n) : 0;
    std::vector<char> z((outs & car::kOutZ) ? rows * esz : 0, (char)0xA5), a((outs & car::kOutA) ? rows * esz : 0, (char)0xA5);
    std::vector<char> e((outs & car::kOutE) ? rows * 8 : 0, (char)0xA5), th((outs & car::kOutT) ? rows * 8 : 0, (char)0xA5);
    CheckedMem m;
    m.rd.push_back({gains.data(), gains.data() + gains.size()});
    m.rd.push_back({r.data(), r.data() + r.size()});
    for (int64_t row = 0; any && row < nrow; ++row) {
        m.rd.push_back({x.data() + (row * x_stride + start) * esz, x.data() + (row * x_stride + span) * esz});
        if (outs & car::kOutZ) m.wr.push_back({z.data() + row * y_stride * esz, z.data() + (row * y_stride + n) * esz});
        if (outs & car::kOutA) m.wr.push_back({a.data() + row * y_stride * esz, a.data() + (row * y_stride + n) * esz});
        if (outs & car::kOutE) m.wr.push_back({e.data() + row * y_stride * 8, e.data() + (row * y_stride + n) * 8});
        if (outs & car::kOutT) m.wr.push_back({th.data() + row * y_stride * 8, th.data() + (row * y_stride + n) * 8});
    }
    std::vector<double> tre(sym::kTab), tim(sym::kTab);
    for (int i = 0; i < (int)(tab.size() / 16); ++i) {
        memcpy(&tre[i], tab.data() + 16 * i, 8);
        memcpy(&tim[i], tab.data() + 16 * i + 8, 8);
    }
    car::Loop lp;
    car::loop_make(fam, mod, open_loop, inv_sqrt2, tre.data(), tim.data(), &lp);
    std::vector<double> image((size_t)p.lds_doubles);
    std::vector<unsigned char> written((size_t)p.lds_doubles);
    const CheckedLds L = {image.data(), written.data(), p.lds_doubles};
    const double *gp = per_row ? reinterpret_cast<const double *>(gains.data()) : nullptr, *rp = fam == sym::kQam ? reinterpret_cast<const double *>(r.data()) : nullptr;
    for (int64_t group = 0; any && group < p.groups; ++group) {
        car::Row w[car::kLane];
        car::State st[car::kLane];
        std::vector<car::Sample> regs((size_t)car::kLane * car::kPer);
        for (int t = 0; t < car::kLane; ++t) {
            w[t] = car::row_of(m, k1, k2, gp, rp, group * car::kLane + t, nrow);
            st[t] = car::State{0.0, 0.0};
        }
        p.c64 ? fetch_all<true>(m, p, x.data(), group, 0, regs) : fetch_all<false>(m, p, x.data(), group, 0, regs);
        for (int64_t tile = 0; tile < p.tiles; ++tile) {
            std::fill(written.begin(), written.end(), 0);
            for (int t = 0; t < car::kLane; ++t) p.c64 ? car::tile_put<true>(p, t, &regs[(size_t)t * car::kPer], L) : car::tile_put<false>(p, t, &regs[(size_t)t * car::kPer], L);
            if (tile + 1 < p.tiles) p.c64 ? fetch_all<true>(m, p, x.data(), group, tile + 1, regs) : fetch_all<false>(m, p, x.data(), group, tile + 1, regs);
            for (int t = 0; t < car::kLane; ++t) {
                if (fam == sym::kQam)
                    walk_type<sym::kQam>(type, p, lp, w[t], group, tile, t, st[t], L);
                else
                    walk_type<sym::kMpsk>(type, p, lp, w[t], group, tile, t, st[t], L);
            }
            for (int t = 0; t < car::kLane; ++t) {
                double *ep = reinterpret_cast<double *>(e.data()), *tp = reinterpret_cast<double *>(th.data());
                p.c64 ? car::tile_store<true>(m, p, z.data(), a.data(), ep, tp, group, tile, t, L) : car::tile_store<false>(m, p, z.data(), a.data(), ep, tp, group, tile, t, L);
            }
        }
    }
    const std::string prefix = v[20];
    if (outs & car::kOutZ) write_file(prefix + "z.bin", z.data(), z.size());
    if (outs & car::kOutA) write_file(prefix + "a.bin", a.data(), a.size());
    if (outs & car::kOutE) write_file(prefix + "e.bin", e.data(), e.size());
    if (outs & car::kOutT) write_file(prefix + "t.bin", th.data(), th.size());
    return 0;
}

static int run_imp(char **v)
{
    const int mode = atoi(v[0]), dtype = atoi(v[1]);
    const int64_t n = atoll(v[2]), n_out = atoll(v[3]), nrow = atoll(v[4]), ns = atoll(v[5]), n_step = atoll(v[6]), x_stride = atoll(v[7]), y_stride = atoll(v[8]);
    const int64_t shift = atoll(v[9]);
    const int per_row = atoi(v[10]);
    const double c = strtod(v[11], nullptr), d = strtod(v[12], nullptr);
    car::ImpPlan p;
    if (const char *why = car::imp_plan_make(mode, dtype, n, n_out, nrow, ns, n_step, x_stride, y_stride, &p)) die(why);
    const int esz = dtype == 1 ? 8 : 16;
    const bool any = n_out > 0 && nrow > 0;
    std::vector<char> vals = read_file(v[13], per_row ? (size_t)nrow * (mode ? 16 : 8) : 0);
    std::vector<char> x = read_file(v[14], nrow > 0 && n > 0 ? (size_t)((nrow - 1) * x_stride + n) * esz : 0);
    std::vector<char> y(any ? (size_t)((nrow - 1) * y_stride + n_out) * esz : 0, (char)0xA5);
    CheckedMem m;
    for (int64_t row = 0; row < nrow; ++row) {
        if (n > 0) m.rd.push_back({x.data() + row * x_stride * esz, x.data() + (row * x_stride + n) * esz});
        if (any) m.wr.push_back({y.data() + row * y_stride * esz, y.data() + (row * y_stride + n_out) * esz});
    }
    for (int64_t row = 0; any && row < nrow; ++row) {
        int64_t sh = shift;
        double cc = c, dd = d;
        if (per_row && mode == 0) memcpy(&sh, vals.data() + 8 * row, 8);
        if (per_row && mode == 1) {
            memcpy(&cc, vals.data() + 16 * row, 8);
            memcpy(&dd, vals.data() + 16 * row + 8, 8);
        }
        for (int64_t j = 0; j < n_out; ++j) car::imp_item(m, p, x.data(), y.data(), row, j, sh, cc, dd);
    }
    write_file(v[15], y.data(), y.size());
    return 0;
}

static int run_funcs(char **v)
{
    const int64_t n = atoll(v[0]);
    std::vector<char> in = read_file(v[1], (size_t)n * 16);
    std::vector<double> out((size_t)n * 6);
    for (int64_t i = 0; i < n; ++i) {
        double a, b;
        memcpy(&a, in.data() + 16 * i, 8);
        memcpy(&b, in.data() + 16 * i + 8, 8);
        car::sincos_rad(a, &out[6 * i], &out[6 * i + 1]);
        out[6 * i + 2] = car::wrap_2pi(a);
        out[6 * i + 3] = sym::atan2_rn(a, b);
        out[6 * i + 4] = car::sign_np(a);
        out[6 * i + 5] = car::cdiv_imag_np(a, b, b, a);
    }
    write_file(v[2], out.data(), out.size() * 8);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "plan") {
        printf("%d %d %d\n", car::kLane, car::kTile, car::kPitch);
        return 0;
    }
    if (cmd == "lds" && argc == 3) {
        car::Plan p;
        if (const char *why = car::plan_make(sym::kMpsk, 4, 0, 3, atoi(argv[2]), 1, 1, 0, 1, 1, 1, &p)) die(why);
        printf("%d\n", p.lds_doubles);
        return 0;
    }
    if (cmd == "funcs" && argc == 5) return run_funcs(argv + 2);
    if (cmd == "rows" && argc == 23) return run_rows(argv + 2);
    if (cmd == "imp" && argc == 18) return run_imp(argv + 2);
    die("usage: plan | lds ... | funcs ... | rows ... | imp ...");
    return 2;
}
