// symerr_emul.cpp -- the symbol-error kernels of csrc/symerr.hip walked thread by thread on the CPU from csrc/symerr_core.hpp: the same plans, index
// algebra, quantiser and per-element functions, with every global access checked against the windows the call owns and every LDS access checked
// against the image (and against reading a word no thread of the workgroup has written).  A stand-alone program: tests/test_symerr_cpu.py builds it
// plain and with -fsanitize=address,undefined and runs it as a child process.
//
//   symerr_emul plan
//   symerr_emul lagplan <len> <n_lags>                                                         K, lags, groups, partitions, tiles per partition, scratch doubles
//   symerr_emul lag <a_dtype> <b_dtype> <len> <n_lags> <quant> <a.bin> <b.bin> <out.bin>      out: nl complex128, then E1, E2
//   symerr_emul cnt <tx_dtype> <tx_stride> <t0> <x_dtype> <x_stride> <start> <step> <r0> <n> <nrow> <mode> <levels> <k> <tx.bin> <x.bin> <out.bin>
// The input files hold exactly the elements the call may read: the buffers are allocated to that size, so a sanitizer sees one element too many.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "symerr_core.hpp"

using namespace skdsp;

static void die(const char *what)
{
    fprintf(stderr, "symerr_emul: %s\n", what);
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
        check(rd, g, 4, "global read outside the window");
        return (double)*g;
    }
    double ld_f64(const double *g) const
    {
        check(rd, g, 8, "global read outside the window");
        return *g;
    }
    void ld_c64(const float *g, double *re, double *im) const
    {
        check(rd, g, 8, "global read outside the window");
        *re = (double)g[0];
        *im = (double)g[1];
    }
    void ld_c128(const double *g, double *re, double *im) const
    {
        check(rd, g, 16, "global read outside the window");
        *re = g[0];
        *im = g[1];
    }
    void ld_f64x2(const double *g, double *a, double *b) const
    {
        check(rd, g, 16, "global read outside the window");
        if ((uintptr_t)g & 15) die("misaligned 16-byte read");
        *a = g[0];
        *b = g[1];
    }
    void st_f64x2(double *g, double a, double b) const
    {
        check(wr, g, 16, "global write outside the window");
        if ((uintptr_t)g & 15) die("misaligned 16-byte write");
        g[0] = a;
        g[1] = b;
    }
};

struct CheckedLds {
    double *w;
    unsigned char *written;
    double ld(int i) const
    {
        if (i < 0 || i >= sye::kLdsDoubles) die("LDS read outside the image");
        if (!written[i]) die("LDS read of a word nobody wrote");
        return w[i];
    }
    void st(int i, double v) const
    {
        if (i < 0 || i >= sye::kLdsDoubles) die("LDS write outside the image");
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

static int run_lag(char **v)
{
    const int a_dtype = atoi(v[0]), b_dtype = atoi(v[1]);
    const int64_t len = atoll(v[2]), n_lags = atoll(v[3]);
    const int quant = atoi(v[4]);
    sye::LagPlan p;
    if (const char *why = sye::lag_plan_make(len, n_lags, a_dtype, b_dtype, quant, &p)) die(why);
    // exactly the K elements a call reads of each stream
    std::vector<char> a = read_file(v[5], (size_t)p.K * sye::elem_bytes(a_dtype)), b = read_file(v[6], (size_t)p.K * sye::elem_bytes(b_dtype));
    std::vector<double> scratch_store((size_t)sye::lag_scratch_doubles(p) + 2), out_store(2 * (size_t)p.nl + 2 + 2);
    double *scratch = scratch_store.data() + (((uintptr_t)scratch_store.data() & 15) ? 1 : 0), *out = out_store.data() + (((uintptr_t)out_store.data() & 15) ? 1 : 0);
    CheckedMem m;
    m.rd = {{a.data(), a.data() + a.size()}, {b.data(), b.data() + b.size()}};
    m.wr = {{(const char *)scratch, (const char *)(scratch + sye::lag_scratch_doubles(p))}};
    std::vector<double> image(sye::kLdsDoubles);
    std::vector<unsigned char> written(sye::kLdsDoubles);
    std::vector<sye::LagAcc> acc(sye::kThreads);
    std::vector<double> e1(sye::kThreads), e2(sye::kThreads);
    for (int part = 0; part < p.nparts; ++part) {
        for (int g = 0; g < p.ngroups; ++g) {
            std::fill(written.begin(), written.end(), 0);
            const CheckedLds L = {image.data(), written.data()};
            for (int t = 0; t < sye::kThreads; ++t) {
                for (int j = 0; j < sye::kRL; ++j) acc[t].re[j] = acc[t].im[j] = 0.0;
                e1[t] = e2[t] = 0.0;
            }
            for (int64_t tile = sye::lag_tile_first(p, part); tile < sye::lag_tile_end(p, part); ++tile) {
                std::fill(written.begin(), written.end(), 0);                 // a tile reads only what ITS staging wrote
                for (int t = 0; t < sye::kThreads; ++t) sye::lag_stage(m, p, a.data(), b.data(), tile, g, t, L);
                for (int t = 0; t < sye::kThreads; ++t) {
                    if (g == 0) sye::lag_energy(p, tile, t, L, &e1[t], &e2[t]);
                    sye::lag_mac(p, g, t, L, acc[t]);
                }
            }
            std::fill(written.begin(), written.end(), 0);
            for (int t = 0; t < sye::kThreads; ++t) sye::lag_put(t, L, acc[t], e1[t], e2[t]);
            for (int t = 0; t < sye::kThreads; ++t) sye::lag_store(m, p, g, part, t, L, scratch);
        }
    }
    // the merge kernel: the grid the launch uses
    CheckedMem mm;
    mm.rd = m.wr;
    mm.wr = {{(const char *)out, (const char *)(out + 2 * p.nl + 2)}};
    const int64_t blocks = (p.nl + 1 + sye::kThreads - 1) / sye::kThreads;
    for (int64_t i = 0; i < blocks * sye::kThreads; ++i) sye::lag_merge_item(mm, p, scratch, i, out, out + 2 * p.nl);
    write_file(v[7], out, (size_t)(2 * p.nl + 2) * sizeof(double));
    printf("%lld %lld %d %d %lld %lld\n", (long long)p.K, (long long)p.nl, p.ngroups, p.nparts, (long long)p.tpp, (long long)p.l0);
    return 0;
}

static int run_cnt(char **v)
{
    const int tx_dtype = atoi(v[0]);
    const int64_t tx_stride = atoll(v[1]), t0 = atoll(v[2]);
    const int x_dtype = atoi(v[3]);
    const int64_t x_stride = atoll(v[4]), start = atoll(v[5]), step = atoll(v[6]), r0 = atoll(v[7]), n = atoll(v[8]), nrow = atoll(v[9]);
    const int mode = atoi(v[10]), levels = atoi(v[11]), k = atoi(v[12]);
    sye::CntPlan p;
    if (const char *why = sye::cnt_plan_make(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, mode, levels, k, &p)) die(why);
    // through the last element a row reads, as the host entry point copies
    const size_t tx_el = n && nrow ? (size_t)((nrow - 1) * tx_stride + t0 + n) : 0, x_el = n && nrow ? (size_t)((nrow - 1) * x_stride + start + (r0 + n - 1) * step + 1) : 0;
    std::vector<char> tx = read_file(v[13], tx_el * sye::elem_bytes(tx_dtype)), x = read_file(v[14], x_el * sye::elem_bytes(x_dtype));
    // a row's own windows only: reads between the rows' windows are errors too
    CheckedMem m;
    for (int64_t r = 0; r < nrow && n; ++r) {
        const char *t_lo = tx.data() + (r * tx_stride + t0) * sye::elem_bytes(tx_dtype);
        m.rd.push_back({t_lo, t_lo + n * sye::elem_bytes(tx_dtype)});
        const char *x_lo = x.data() + (r * x_stride + sye::cnt_x_at(p, 0)) * sye::elem_bytes(x_dtype);
        m.rd.push_back({x_lo, x_lo + ((n - 1) * step + 1) * sye::elem_bytes(x_dtype)});
    }
    std::vector<int64_t> counts((size_t)(4 * nrow));
    const int64_t items = sye::cnt_items_per_row(n);
    for (int64_t blk = 0; blk < items * nrow; ++blk) {
        const int64_t row = blk / items, it = blk - row * items;
        for (int t = 0; t < sye::kThreads; ++t) {
            sye::Cnt c = {{0, 0, 0, 0}};
            sye::cnt_thread(m, p, tx.data() + row * tx_stride * sye::elem_bytes(tx_dtype), x.data() + row * x_stride * sye::elem_bytes(x_dtype), it, t, c);
            for (int q = 0; q < 4; ++q) counts[(size_t)(4 * row + q)] += c.c[q];
        }
    }
    write_file(v[15], counts.data(), counts.size() * sizeof(int64_t));
    return 0;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "plan") {
        printf("%d %d %d %d %d %d %d\n", sye::kThreads, sye::kLagsWg, sye::kTile, sye::kWin, sye::kTargetWgs, sye::kMaxParts, sye::kSymWg);
        return 0;
    }
    if (cmd == "lagplan" && argc == 4) {
        sye::LagPlan p;
        if (const char *why = sye::lag_plan_make(atoll(argv[2]), atoll(argv[3]), 0, 0, 0, &p)) die(why);
        printf("%lld %lld %d %d %lld %lld\n", (long long)p.K, (long long)p.nl, p.ngroups, p.nparts, (long long)p.tpp, (long long)sye::lag_scratch_doubles(p));
        return 0;
    }
    if (cmd == "lag" && argc == 10) return run_lag(argv + 2);
    if (cmd == "cnt" && argc == 18) return run_cnt(argv + 2);
    die("usage: plan | lag ... | cnt ...");
    return 2;
}
