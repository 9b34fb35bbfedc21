// Host emulation of the OFDM kernels (no GPU): csrc/ofdm_core.hpp's per-thread phases run thread by thread and pass by pass exactly as
// csrc/ofdm.hip schedules them, over rows in exact-size allocations; every global access is checked against the row's window and its
// alignment (exit code 9 and a message otherwise).
//   ofdm_emul pos                                                                     pos_of(bin_of(p)) == p for every p of every size; the geometry
//   ofdm_emul tx dtype nsym nrow nf nc npb cp ncp xoff yoff x.bin y.bin               dtype 1 complex64, 3 complex128
//   ofdm_emul rx dtype nsym nrow nf nc npb cp ncp alpha has_ht xoff zoff x.bin hht.f64 z.bin h.bin
//   ofdm_emul eq dtype nsym nrow nf npb alpha has_ht z.bin hht.f64 out.bin h.bin       chan_est_equalize on rows of z ([nsym, nf], back to back)
// Rows are stride = row length + 1 elements apart behind xoff / yoff / zoff elements, so windows start off a 16-byte boundary where asked; the
// outputs are written whole, with 0xEE in every byte no kernel wrote.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I scikit-dsp-comm_amd/csrc tests/host/ofdm_emul.cpp -o /tmp/ofdm_emul
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ofdm_core.hpp"

using namespace skdsp::ofdm;

struct Range {
    const char *lo, *hi;
};
struct Mem {
    std::vector<Range> rd, wr;
    static void check(const std::vector<Range> &rs, const void *p, size_t bytes, size_t align, const char *what)
    {
        const char *c = static_cast<const char *>(p);
        if ((uintptr_t)c % align) {
            std::fprintf(stderr, "misaligned %s of %zu bytes\n", what, bytes);
            std::exit(9);
        }
        for (const Range &r : rs)
            if (c >= r.lo && c + bytes <= r.hi) return;
        std::fprintf(stderr, "%s of %zu bytes outside the row's window\n", what, bytes);
        std::exit(9);
    }
    cx<double> ld(const float *g) const
    {
        check(rd, g, 8, 8, "load");
        return cx<double>{(double)g[0], (double)g[1]};
    }
    cx<double> ld(const double *g) const
    {
        check(rd, g, 16, 16, "load");
        return cx<double>{g[0], g[1]};
    }
    cx<double> ld_tab(const cx<double> *tab, int i) const
    {
        check(rd, tab + i, 16, 16, "table load");
        return tab[i];
    }
    void st(float *g, cx<double> v) const
    {
        check(wr, g, 8, 8, "store");
        g[0] = (float)v.x;
        g[1] = (float)v.y;
    }
    void st(double *g, cx<double> v) const
    {
        check(wr, g, 16, 16, "store");
        g[0] = v.x;
        g[1] = v.y;
    }
    void st2(float *g, cx<double> a, cx<double> b) const
    {
        check(wr, g, 16, 16, "paired store");
        g[0] = (float)a.x;
        g[1] = (float)a.y;
        g[2] = (float)b.x;
        g[3] = (float)b.y;
    }
};

template <typename T> static Range range_of(const T *p, long long scalars) { return Range{(const char *)p, (const char *)(p + scalars)}; }

static void *exact_alloc(size_t bytes, int fill)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1)) std::exit(7);
    std::memset(p, fill, bytes);
    return p;
}
static void read_file(const char *name, void *dst, size_t bytes)
{
    FILE *f = std::fopen(name, "rb");
    if (!f || (bytes && std::fread(dst, 1, bytes, f) != bytes)) std::exit(3);
    std::fclose(f);
}
static void write_file(const char *name, const void *src, size_t bytes)
{
    FILE *f = std::fopen(name, "wb");
    if (!f || (bytes && std::fwrite(src, 1, bytes, f) != bytes)) std::exit(6);
    std::fclose(f);
}

template <int LOG2N> static std::vector<cx<double>> twiddles()
{
    const int N = 1 << LOG2N;
    const double kTwoPi = 6.283185307179586476925286766559;
    std::vector<cx<double>> tw(N);
    for (int i = 0; i < N; ++i) tw[i] = cx<double>{std::cos(kTwoPi * i / N), -std::sin(kTwoPi * i / N)};
    return tw;
}

// passes 1 .. of the group's transforms, all threads of a pass before the next one (a barrier in between)
template <int LOG2N> static void transform_rest(const cx<double> *tw, cx<double> *work)
{
    typedef Core<LOG2N> C;
    for (int s = 1; s < C::NSTORE; ++s)
        for (int tid = 0; tid < kThreads; ++tid) C::mid(s, tid % C::TS, tw, work + (tid / C::TS) * C::N);
    for (int tid = 0; tid < kThreads; ++tid) C::last_store(tid % C::TS, work + (tid / C::TS) * C::N);
}

template <typename S, int LOG2N> static void run_tx(const S *x, S *y, const TxPlan &p, long long nrow)
{
    typedef Core<LOG2N> C;
    const std::vector<cx<double>> tw = twiddles<LOG2N>();
    std::vector<cx<double>> work((size_t)C::NB * C::N);
    for (long long it = 0; it < p.groups * nrow; ++it) {
        const long long row = it / p.groups, j0 = (it - row * p.groups) * C::NB;
        const S *xrow = x + 2 * row * p.x_stride;
        S *yrow = y + 2 * row * p.y_stride;
        Mem mem;
        mem.rd.push_back(range_of(xrow, 2 * p.nsym * p.nf));
        mem.wr.push_back(range_of(yrow, 2 * p.T * (p.nc + p.ncp)));
        for (int tid = 0; tid < kThreads; ++tid) tx_first<S, LOG2N>(mem, p, xrow, j0, tid, tw.data(), work.data());
        transform_rest<LOG2N>(tw.data(), work.data());
        for (int tid = 0; tid < kThreads; ++tid) tx_store<S, LOG2N>(mem, p, yrow, j0, tid, work.data());
    }
}

template <typename SI, typename SO, int LOG2N>
static void run_rx(const SI *x, SO *z, double *pil, const cx<double> *hht, const RxPlan &p, long long nrow)
{
    typedef Core<LOG2N> C;
    const std::vector<cx<double>> tw = twiddles<LOG2N>();
    std::vector<cx<double>> work((size_t)C::NB * C::N);
    for (long long it = 0; it < p.groups * nrow; ++it) {
        const long long row = it / p.groups, k0 = (it - row * p.groups) * C::NB;
        const SI *xrow = x + 2 * row * p.x_stride;
        SO *zrow = z + 2 * row * p.z_stride;
        double *prow = pil + 2 * row * p.npilot * p.nf;
        Mem mem;
        mem.rd.push_back(range_of(xrow, 2 * p.nsym * p.stride));
        if (hht) mem.rd.push_back(range_of(hht, p.nf));
        mem.wr.push_back(range_of(zrow, 2 * p.ndata * p.nf));
        mem.wr.push_back(range_of(prow, 2 * p.npilot * p.nf));
        for (int tid = 0; tid < kThreads; ++tid) rx_first<SI, LOG2N>(mem, p, xrow, k0, tid, tw.data(), work.data());
        transform_rest<LOG2N>(tw.data(), work.data());
        for (int tid = 0; tid < kThreads; ++tid) rx_store<SO, LOG2N>(mem, p, zrow, prow, hht, k0, tid, work.data());
    }
}

template <typename SI>
static void run_chanest(const SI *src, long long src_stride, long long pitch, long long npilot, long long nrow, int nf, double alpha, double *est, double *h)
{
    for (long long row = 0; row < nrow; ++row) {
        const SI *s = src + 2 * row * src_stride;
        double *e = est + 2 * row * npilot * nf, *hr = h + 2 * row * nf;
        Mem mem;
        mem.rd.push_back(range_of(s, 2 * ((npilot - 1) * pitch + nf)));
        mem.wr.push_back(range_of(e, 2 * npilot * nf));
        mem.wr.push_back(range_of(hr, 2 * nf));
        for (int c = 0; c < nf; ++c) chanest_item<SI>(mem, s, pitch, npilot, nf, c, alpha, e, hr);
    }
}

template <typename SI, typename SO>
static void run_equalize(const SI *src, long long src_stride, int compact, const double *est, const cx<double> *hht, long long npilot, long long ndata, long long nrow,
                         int nf, int npb, SO *out, long long out_stride)
{
    for (long long row = 0; row < nrow; ++row) {
        const SI *s = src + 2 * row * src_stride;
        const double *e = est + 2 * row * npilot * nf;
        SO *o = out + 2 * row * out_stride;
        Mem mem;
        mem.rd.push_back(range_of(s, 2 * (compact ? ndata : ndata + npilot) * nf));
        mem.rd.push_back(range_of(e, 2 * npilot * nf));
        if (hht) mem.rd.push_back(range_of(hht, nf));
        mem.wr.push_back(range_of(o, 2 * ndata * nf));
        for (long long el = 0; el < ndata * nf; ++el) equalize_item<SI, SO>(mem, s, compact, e, hht, nf, npb, el, o);
    }
}

#define BY_LOG2(call, ...)                                \
    switch (log2_of(nc)) {                                \
    case 6: call<__VA_ARGS__, 6> ARGS; break;             \
    case 7: call<__VA_ARGS__, 7> ARGS; break;             \
    case 8: call<__VA_ARGS__, 8> ARGS; break;             \
    case 9: call<__VA_ARGS__, 9> ARGS; break;             \
    case 10: call<__VA_ARGS__, 10> ARGS; break;           \
    case 11: call<__VA_ARGS__, 11> ARGS; break;           \
    default: call<__VA_ARGS__, 12> ARGS; break;           \
    }

template <int LOG2N> static int check_pos()
{
    typedef Core<LOG2N> C;
    for (int p = 0; p < C::N; ++p)
        if (C::pos_of(C::bin_of(p)) != p || C::bin_of(C::pos_of(p)) != p) return 1;
    std::printf("%d %d %d\n", C::N, C::NB, C::R);
    return 0;
}

template <typename S> static int main_tx(char **a)
{
    const long long nsym = std::atoll(a[3]), nrow = std::atoll(a[4]);
    const int nf = std::atoi(a[5]), nc = std::atoi(a[6]), npb = std::atoi(a[7]), cp = std::atoi(a[8]), ncp = std::atoi(a[9]);
    const long long xoff = std::atoll(a[10]), yoff = std::atoll(a[11]);
    if (shape_why(nf, nc, npb, ncp, 0, 0)) return 5;
    const long long n_in = nsym * nf, n_out = tx_symbols(nsym, npb) * (nc + (cp ? ncp : 0)), xs = n_in + 1, ys = n_out + 1;
    const size_t xel = (size_t)(xoff + (nrow - 1) * xs + n_in), yel = (size_t)(yoff + (nrow - 1) * ys + n_out), esz = 2 * sizeof(S);
    S *xb = (S *)exact_alloc(xel * esz, 0), *yb = (S *)exact_alloc(yel * esz, 0xEE);
    read_file(a[12], xb + 2 * xoff, (xel - xoff) * esz);
    TxPlan p;
    tx_plan_make(nsym, nf, nc, npb, cp, ncp, xs, ys, &p);
#define ARGS (xb + 2 * xoff, yb + 2 * yoff, p, nrow)
    BY_LOG2(run_tx, S)
#undef ARGS
    write_file(a[13], yb, yel * esz);
    std::free(xb);
    std::free(yb);
    return 0;
}

template <typename S> static int main_rx(char **a)
{
    const long long nsym = std::atoll(a[3]), nrow = std::atoll(a[4]);
    const int nf = std::atoi(a[5]), nc = std::atoi(a[6]), npb = std::atoi(a[7]), cp = std::atoi(a[8]), ncp = std::atoi(a[9]);
    const double alpha = std::atof(a[10]);
    const int has_ht = std::atoi(a[11]);
    const long long xoff = std::atoll(a[12]), zoff = std::atoll(a[13]);
    if (shape_why(nf, nc, npb, ncp, 1, has_ht)) return 5;
    RxPlan p;
    rx_plan_make(nsym, nf, nc, npb, cp, ncp, 0, 0, &p);
    const long long n_in = nsym * p.stride, n_out = p.ndata * nf, xs = n_in + 1, zs = n_out + 1;
    p.x_stride = xs;
    p.z_stride = zs;
    const size_t xel = (size_t)(xoff + (nrow - 1) * xs + n_in), zel = (size_t)(zoff + (nrow - 1) * zs + n_out), esz = 2 * sizeof(S);
    S *xb = (S *)exact_alloc(xel * esz, 0), *zb = (S *)exact_alloc(zel * esz, 0xEE);
    read_file(a[14], xb + 2 * xoff, (xel - xoff) * esz);
    cx<double> *hht = nullptr;
    if (has_ht && npb != 0) {
        hht = (cx<double> *)exact_alloc((size_t)nf * 16, 0);
        read_file(a[15], hht, (size_t)nf * 16);
    }
    double *pil = (double *)exact_alloc((size_t)nrow * p.npilot * nf * 16, 0xEE), *rawz = (double *)exact_alloc((size_t)nrow * p.ndata * nf * 16, 0xEE);
    double *h = (double *)exact_alloc((size_t)nrow * nf * 16, 0xEE);
    const bool raw = npb > 0 && !has_ht;
    if (raw) {
        p.z_stride = p.ndata * nf;
#define ARGS (xb + 2 * xoff, rawz, pil, hht, p, nrow)
        BY_LOG2(run_rx, S, double)
#undef ARGS
    } else {
#define ARGS (xb + 2 * xoff, zb + 2 * zoff, pil, hht, p, nrow)
        BY_LOG2(run_rx, S, S)
#undef ARGS
    }
    if (npb > 0) {
        run_chanest<double>(pil, p.npilot * nf, nf, p.npilot, nrow, nf, alpha, pil, h);
        if (raw) run_equalize<double, S>(rawz, p.ndata * nf, 1, pil, nullptr, p.npilot, p.ndata, nrow, nf, npb, zb + 2 * zoff, zs);
    }
    write_file(a[16], zb, zel * esz);
    write_file(a[17], h, (size_t)nrow * nf * 16);
    std::free(xb);
    std::free(zb);
    std::free(hht);
    std::free(pil);
    std::free(rawz);
    std::free(h);
    return 0;
}

template <typename S> static int main_eq(char **a)
{
    const long long nsym = std::atoll(a[3]), nrow = std::atoll(a[4]);
    const int nf = std::atoi(a[5]), npb = std::atoi(a[6]);
    const double alpha = std::atof(a[7]);
    const int has_ht = std::atoi(a[8]);
    if (npb < 2 || nsym < 1) return 5;
    const long long npilot = rx_pilots(nsym, npb), ndata = nsym - npilot;
    const size_t esz = 2 * sizeof(S);
    S *zb = (S *)exact_alloc((size_t)nrow * nsym * nf * esz, 0), *ob = (S *)exact_alloc((size_t)nrow * ndata * nf * esz, 0xEE);
    read_file(a[9], zb, (size_t)nrow * nsym * nf * esz);
    cx<double> *hht = nullptr;
    if (has_ht) {
        hht = (cx<double> *)exact_alloc((size_t)nf * 16, 0);
        read_file(a[10], hht, (size_t)nf * 16);
    }
    double *est = (double *)exact_alloc((size_t)nrow * npilot * nf * 16, 0xEE), *h = (double *)exact_alloc((size_t)nrow * nf * 16, 0xEE);
    run_chanest<S>(zb, nsym * nf, (long long)npb * nf, npilot, nrow, nf, alpha, est, h);
    run_equalize<S, S>(zb, nsym * nf, 0, est, hht, npilot, ndata, nrow, nf, npb, ob, ndata * nf);
    write_file(a[11], ob, (size_t)nrow * ndata * nf * esz);
    write_file(a[12], h, (size_t)nrow * nf * 16);
    std::free(zb);
    std::free(ob);
    std::free(hht);
    std::free(est);
    std::free(h);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "pos") return check_pos<6>() | check_pos<7>() | check_pos<8>() | check_pos<9>() | check_pos<10>() | check_pos<11>() | check_pos<12>();
    if (argc < 3) return 2;
    const int dtype = std::atoi(argv[2]);
    if (dtype != 1 && dtype != 3) return 2;
    int rc = 2;
    if (cmd == "tx" && argc == 14) rc = dtype == 1 ? main_tx<float>(argv) : main_tx<double>(argv);
    if (cmd == "rx" && argc == 18) rc = dtype == 1 ? main_rx<float>(argv) : main_rx<double>(argv);
    if (cmd == "eq" && argc == 13) rc = dtype == 1 ? main_eq<float>(argv) : main_eq<double>(argv);
    if (rc == 0) std::printf("OK\n");
    return rc;
}
