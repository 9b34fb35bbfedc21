// pulse_emul.cpp -- the pulse shaping and matched filter kernels of csrc/pulse.hip walked thread by thread on the CPU from csrc/pulse_core.hpp: the same
// plans, index algebra and arithmetic, with every global access checked against the rows the call owns and every LDS access checked against the image
// (and against reading a word no thread of the workgroup has written).  A stand-alone program: tests/test_pulse_cpu.py builds it plain and with
// -fsanitize=address,undefined and runs it as a child process.
//
//   pulse_emul plan                                                threads, shaping tile outputs, matched-filter tile span, max taps, max rate
//   pulse_emul shapeplan <dtype> <ntaps> <ns> <n>                  J, H, T, tiles per row, LDS doubles
//   pulse_emul mfplan <dtype> <ntaps> <n> <start> <step> <naive>   R, To, W, Wq, tiles per row, LDS doubles, n_out
//   pulse_emul shape <dtype> <ntaps> <ns> <n> <nrow> <x_stride> <y_stride> <has_scale> <scale> <b.bin> <x.bin> <y.bin>
//   pulse_emul mf <dtype> <ntaps> <n> <nrow> <start> <step> <x_stride> <y_stride> <naive> <fma> <b.bin> <x.bin> <y.bin>
// x.bin holds exactly the elements from the first row's first to the last row's last; the buffers are allocated to that size, so a sanitizer sees one
// element too many.  y.bin receives the whole output block, (nrow - 1) y_stride + the row length elements, filled with the byte 0xA5 before the walk: the
// gaps between the rows must come back as they were.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pulse_core.hpp"

using namespace skdsp;

static void die(const char *what)
{
    fprintf(stderr, "pulse_emul: %s\n", what);
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
    double ld_f32(const float *g) const
    {
        check(rd, g, 4, "global read outside the rows");
        return (double)*g;
    }
    double ld_f64(const double *g) const
    {
        check(rd, g, 8, "global read outside the rows");
        return *g;
    }
    void ld_c64(const float *g, double *re, double *im) const
    {
        check(rd, g, 8, "global read outside the rows");
        *re = (double)g[0];
        *im = (double)g[1];
    }
    void ld_c128(const double *g, double *re, double *im) const
    {
        check(rd, g, 16, "global read outside the rows");
        *re = g[0];
        *im = g[1];
    }
    void st_f32(float *g, float v) const
    {
        check(wr, g, 4, "global write outside the rows");
        *g = v;
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
static void write_file(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) die("cannot write the output file");
    fclose(f);
}

// the windows a call owns: row r of x is [r x_stride, r x_stride + nx), of y [r y_stride, r y_stride + ny); the taps
static void own_rows(CheckedMem &m, const std::vector<char> &b, const std::vector<char> &x, int64_t x_stride, int64_t nx, std::vector<char> &y, int64_t y_stride, int64_t ny,
                     int64_t nrow, int esz)
{
    m.rd.push_back({b.data(), b.data() + b.size()});
    for (int64_t r = 0; r < nrow; ++r) {
        m.rd.push_back({x.data() + r * x_stride * esz, x.data() + (r * x_stride + nx) * esz});
        m.wr.push_back({y.data() + r * y_stride * esz, y.data() + (r * y_stride + ny) * esz});
    }
}

static int run_shape(char **v)
{
    const int dtype = atoi(v[0]), ntaps = atoi(v[1]);
    const int64_t ns = atoll(v[2]), n = atoll(v[3]), nrow = atoll(v[4]), x_stride = atoll(v[5]), y_stride = atoll(v[6]);
    const int has_scale = atoi(v[7]);
    const double scale = strtod(v[8], nullptr);
    if (!pls::served(ns, ntaps)) die("outside the served range");
    pls::ShapePlan p;
    if (const char *why = pls::shape_plan_make(dtype, ntaps, ns, n, nrow, x_stride, y_stride, has_scale, scale, &p)) die(why);
    const int esz = pls::elem_bytes(dtype);
    const bool any = n > 0 && nrow > 0;
    std::vector<char> b = read_file(v[9], (size_t)ntaps * 8), x = read_file(v[10], any ? (size_t)((nrow - 1) * x_stride + n) * esz : 0);
    std::vector<char> y(any ? (size_t)((nrow - 1) * y_stride + n * ns) * esz : 0, (char)0xA5);
    CheckedMem m;
    own_rows(m, b, x, x_stride, n, y, y_stride, n * ns, any ? nrow : 0, esz);
    std::vector<double> image((size_t)p.lds_doubles);
    std::vector<unsigned char> written((size_t)p.lds_doubles);
    const CheckedLds L = {image.data(), written.data(), p.lds_doubles};
    for (int64_t blk = 0; any && blk < p.tiles * nrow; ++blk) {
        const int64_t row = blk / p.tiles, tile = blk - row * p.tiles;
        std::fill(written.begin(), written.end(), 0);
        for (int t = 0; t < pls::kThreads; ++t) pls::shape_stage(m, p, reinterpret_cast<const double *>(b.data()), x.data() + row * x_stride * esz, tile, t, L);
        for (int t = 0; t < pls::kThreads; ++t) pls::shape_outputs(m, p, y.data() + row * y_stride * esz, tile, t, L);
    }
    write_file(v[11], y.data(), y.size());
    return 0;
}

template <bool FMA> static void mf_walk(const CheckedMem &m, const pls::MfPlan &p, void *y_row, int64_t tile, const CheckedLds &L)
{
    for (int t = 0; t < pls::kThreads; ++t) {
        if (p.R == 4)
            p.cplx ? pls::mf_outputs<4, FMA, true>(m, p, y_row, tile, t, L) : pls::mf_outputs<4, FMA, false>(m, p, y_row, tile, t, L);
        else if (p.R == 2)
            p.cplx ? pls::mf_outputs<2, FMA, true>(m, p, y_row, tile, t, L) : pls::mf_outputs<2, FMA, false>(m, p, y_row, tile, t, L);
        else
            p.cplx ? pls::mf_outputs<1, FMA, true>(m, p, y_row, tile, t, L) : pls::mf_outputs<1, FMA, false>(m, p, y_row, tile, t, L);
    }
}

static int run_mf(char **v)
{
    const int dtype = atoi(v[0]), ntaps = atoi(v[1]);
    const int64_t n = atoll(v[2]), nrow = atoll(v[3]), start = atoll(v[4]), step = atoll(v[5]), x_stride = atoll(v[6]), y_stride = atoll(v[7]);
    const int naive = atoi(v[8]), fma = atoi(v[9]);
    if (!pls::served(step, ntaps)) die("outside the served range");
    pls::MfPlan p;
    if (const char *why = pls::mf_plan_make(dtype, ntaps, n, nrow, start, step, x_stride, y_stride, naive, &p)) die(why);
    const int esz = pls::elem_bytes(dtype);
    const bool any = p.n_out > 0 && nrow > 0;
    std::vector<char> b = read_file(v[10], (size_t)ntaps * 8), x = read_file(v[11], nrow > 0 && n > 0 ? (size_t)((nrow - 1) * x_stride + n) * esz : 0);
    std::vector<char> y(any ? (size_t)((nrow - 1) * y_stride + p.n_out) * esz : 0, (char)0xA5);
    CheckedMem m;
    own_rows(m, b, x, x_stride, n, y, y_stride, p.n_out, any ? nrow : 0, esz);
    std::vector<double> image((size_t)p.lds_doubles);
    std::vector<unsigned char> written((size_t)p.lds_doubles);
    const CheckedLds L = {image.data(), written.data(), p.lds_doubles};
    for (int64_t blk = 0; any && blk < p.tiles * nrow; ++blk) {
        const int64_t row = blk / p.tiles, tile = blk - row * p.tiles;
        std::fill(written.begin(), written.end(), 0);
        for (int t = 0; t < pls::kThreads; ++t) pls::mf_stage(m, p, reinterpret_cast<const double *>(b.data()), x.data() + row * x_stride * esz, tile, t, L);
        if (fma)
            mf_walk<true>(m, p, y.data() + row * y_stride * esz, tile, L);
        else
            mf_walk<false>(m, p, y.data() + row * y_stride * esz, tile, L);
    }
    write_file(v[12], y.data(), y.size());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "plan") {
        printf("%d %d %d %d %d\n", pls::kThreads, pls::kShapeOut, pls::kMfIn, pls::kMaxTaps, pls::kMaxRate);
        return 0;
    }
    if (cmd == "shapeplan" && argc == 6) {
        pls::ShapePlan p;
        if (!pls::served(atoll(argv[4]), atoll(argv[3]))) die("outside the served range");
        if (const char *why = pls::shape_plan_make(atoi(argv[2]), atoi(argv[3]), atoll(argv[4]), atoll(argv[5]), 1, atoll(argv[5]), atoll(argv[5]) * atoll(argv[4]), 0, 1.0, &p))
            die(why);
        printf("%d %d %d %lld %d\n", p.J, p.H, p.T, (long long)p.tiles, p.lds_doubles);
        return 0;
    }
    if (cmd == "mfplan" && argc == 8) {
        pls::MfPlan p;
        const int64_t n = atoll(argv[4]), start = atoll(argv[5]), step = atoll(argv[6]);
        if (!pls::served(step, atoll(argv[3]))) die("outside the served range");
        if (const char *why = pls::mf_plan_make(atoi(argv[2]), atoi(argv[3]), n, 1, start, step, n, pls::mf_out_len(n, start, step), atoi(argv[7]), &p)) die(why);
        printf("%d %d %d %d %lld %d %lld\n", p.R, p.To, p.W, p.Wq, (long long)p.tiles, p.lds_doubles, (long long)p.n_out);
        return 0;
    }
    if (cmd == "shape" && argc == 14) return run_shape(argv + 2);
    if (cmd == "mf" && argc == 15) return run_mf(argv + 2);
    die("usage: plan | shapeplan ... | mfplan ... | shape ... | mf ...");
    return 2;
}
