// Host emulation of the FEC chain kernels (no GPU): csrc/convcode_core.hpp's plans, staging and per-item functions, walked work item by
// work item and thread by thread exactly as csrc/convcode.hip schedules them.
//   convcode_emul plan
//       "run R wg W cnt_wg C gather_item G threads T": bits per lane / per work item of the encoder, bytes per item of the count,
//       elements per item of the gathers
//   convcode_emul len dep n pat1 pat2
//       the output elements per row of puncture (dep 0) / depuncture (dep 1)
//   convcode_emul enc G1,G2[,G3] n nrow nstates states_in.u8 in.u8 out.u8 states_out.u8 in_off out_off
//   convcode_emul gat dep n nrow elem_bytes pat1 pat2 erase_hex in.bin out.bin in_off out_off        (offsets in elements)
//   convcode_emul cnt n nrow tx_stride rx_stride invert tx.u8 rx.u8 tx_off rx_off                    ("count count ..." on stdout)
// Each input window sits `off` bytes into an allocation of exactly off + len bytes whose head is 0xFF, each output window behind a guard
// that must survive; every global access is checked against its window (exit 7) and every LDS image is an allocation of exactly the
// kernel's bytes, so -fsanitize=address sees what the checks cannot.
// Build: g++ -O1 -std=c++17 -I scikit-dsp-comm_amd/csrc tests/host/convcode_emul.cpp -o /tmp/convcode_emul
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "convcode_core.hpp"

using namespace skdsp;
using namespace skdsp::cvc;

struct Window {
    const uint8_t *lo, *hi;
    void need(const void *q, int bytes) const
    {
        const uint8_t *p = static_cast<const uint8_t *>(q);
        if (p < lo || p + bytes > hi) {
            fprintf(stderr, "access of %d bytes at window offset %lld outside [0, %lld)\n", bytes, (long long)(p - lo), (long long)(hi - lo));
            exit(7);
        }
    }
};
struct HostMem {
    Window in, in2, out;
    uint8_t ld8(const uint8_t *g) const
    {
        if (g >= in2.lo && g < in2.hi) in2.need(g, 1);
        else in.need(g, 1);
        return *g;
    }
    void st8(uint8_t *g, uint8_t v) const { out.need(g, 1); *g = v; }
    void in16(uint8_t *img, const uint8_t *g) const
    {
        if (g >= in2.lo && g < in2.hi) in2.need(g, 16);
        else in.need(g, 16);
        if (((uintptr_t)g | (uintptr_t)img) & 15) { fprintf(stderr, "unaligned 16-byte load\n"); exit(8); }
        memcpy(img, g, 16);
    }
    void out16(uint8_t *g, const uint8_t *img) const
    {
        out.need(g, 16);
        if (((uintptr_t)g | (uintptr_t)img) & 15) { fprintf(stderr, "unaligned 16-byte store\n"); exit(8); }
        memcpy(g, img, 16);
    }
    template <typename T> T ld(const T *g) const
    {
        in.need(g, sizeof(T));
        if ((uintptr_t)g % sizeof(T)) { fprintf(stderr, "unaligned element load\n"); exit(8); }
        return *g;
    }
    template <typename T> void st(T *g, T v) const
    {
        out.need(g, sizeof(T));
        if ((uintptr_t)g % sizeof(T)) { fprintf(stderr, "unaligned element store\n"); exit(8); }
        *g = v;
    }
};

static std::vector<uint8_t> read_all(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(4);
    uint8_t b[4096];
    size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}
static void write_all(const char *path, const uint8_t *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) exit(4);
    if (n) fwrite(p, 1, n, f);
    fclose(f);
}
static uint64_t mask_of(const char *pat)
{
    uint64_t m = 0;
    for (int k = 0; pat[k] && k < 64; ++k)
        if (pat[k] == '1') m |= (uint64_t)1 << k;
    return m;
}

// an input window `off` bytes into an exact allocation (head 0xFF) / an output window behind a guard head (0xA5), filled with 0xEE
struct Buf {
    uint8_t *base;
    size_t off, len;
    Buf(size_t off_, size_t len_, const uint8_t *src) : off(off_), len(len_)
    {
        base = new uint8_t[off + len + 0];
        if ((uintptr_t)base & 15) exit(9);   // the offsets are meant relative to a 16-byte boundary
        memset(base, src ? 0xFF : 0xA5, off);
        if (src) memcpy(base + off, src, len);
        else memset(base + off, 0xEE, len);
    }
    ~Buf() { delete[] base; }
    uint8_t *win() const { return base + off; }
    Window window() const { return Window{base + off, base + off + len}; }
    void guard_ok() const
    {
        for (size_t i = 0; i < off; ++i)
            if (base[i] != 0xA5) {
                fprintf(stderr, "guard byte %zu in front of the output window was overwritten\n", i);
                exit(7);
            }
    }
};
static uint8_t *lds_alloc(int bytes)
{
    uint8_t *p = new uint8_t[bytes];
    if ((uintptr_t)p & 15) exit(9);
    memset(p, 0xCD, bytes);   // nothing may depend on what the LDS held
    return p;
}

static int run_enc(char **v)
{
    std::vector<std::string> polys;
    std::string all = v[0];
    for (size_t a = 0; a <= all.size();) {
        const size_t b = all.find(',', a) == std::string::npos ? all.size() : all.find(',', a);
        polys.push_back(all.substr(a, b - a));
        a = b + 1;
    }
    const char *cp[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < polys.size() && i < 4; ++i) cp[i] = polys[i].c_str();
    EncPlan p;
    const char *why = enc_plan_make(cp, (int)polys.size(), &p);
    if (why) {
        fprintf(stderr, "%s\n", why);
        return 5;
    }
    const int64_t n = atoll(v[1]), nrow = atoll(v[2]), nstates = atoll(v[3]);
    const std::vector<uint8_t> states = read_all(v[4]), bits = read_all(v[5]);
    const int in_off = atoi(v[8]), out_off = atoi(v[9]);
    if ((int64_t)bits.size() != n * nrow || (int64_t)states.size() != nstates || !(nstates == 0 || nstates == 1 || nstates == nrow)) return 6;
    const int R = p.R;
    Buf in(in_off, bits.size(), bits.data()), out(out_off, bits.size() * R, nullptr);
    std::vector<uint8_t> states_out((size_t)nrow, 0xEE);
    HostMem mem;
    mem.in = in.window();
    mem.in2 = Window{nullptr, nullptr};
    mem.out = out.window();
    const int64_t items = enc_items_per_row(n);
    for (int64_t row = 0; row < nrow; ++row)
        for (int64_t it = 0; it < items; ++it) {
            uint8_t *img_in = lds_alloc(kEncInBytes), *img_out = lds_alloc(blk::image_bytes(R * kEncWg));
            const int len = enc_len(n, it), h = enc_hist(p, it);
            const uint8_t *gin = in.win() + row * n + enc_first(it) - h;
            uint8_t *gout = out.win() + (row * n + enc_first(it)) * R;
            for (int t = 0; t < kThreads; ++t) blk::stage_in(mem, gin, h + len, img_in, t, kThreads);
            // ---- barrier
            for (int t = 0; t < kThreads; ++t) {
                const int i0 = kEncRun * t;
                if (i0 >= len) continue;
                uint32_t state = 0;
                if (it == 0 && t == 0 && nstates) state = states[nstates == nrow && nrow > 1 ? row : 0] & ((1u << (p.K - 1)) - 1u);
                const uint32_t w = enc_lane_word(p, img_in, blk::lead_of(gin), h, len, i0, state);
                const int cnt = len - i0 < kEncRun ? len - i0 : kEncRun;
                enc_put(p, w, cnt, img_out + blk::lead_of(gout) + R * i0);
                if (i0 + cnt == len && it + 1 == items) states_out[row] = (uint8_t)enc_state_after(p, w, cnt - 1);
            }
            // ---- barrier
            for (int t = 0; t < kThreads; ++t) blk::stage_out(mem, gout, R * len, img_out, t, kThreads);
            delete[] img_in;
            delete[] img_out;
        }
    out.guard_ok();
    write_all(v[6], out.win(), out.len);
    write_all(v[7], states_out.data(), states_out.size());
    return 0;
}

template <typename T> static void gather_rows(const HostMem &mem, const GatherPlan &g, const uint8_t *x, uint8_t *y, int64_t n, int64_t n_out, int64_t nrow, uint64_t erase)
{
    const int64_t items = gather_items_per_row(n_out);
    for (int64_t row = 0; row < nrow; ++row)
        for (int64_t it = 0; it < items; ++it) {
            uint8_t *tab = lds_alloc(2 * kMaxPattern);
            memcpy(tab, g.tab, 2 * kMaxPattern);   // thread 0, word by word
            // ---- barrier
            for (int t = 0; t < kThreads; ++t)
                gather_thread<T>(mem, tab, g.p_in, g.p_out, reinterpret_cast<const T *>(x) + row * n, reinterpret_cast<T *>(y) + row * n_out, n_out, (T)erase,
                                 (uint32_t)it, t);
            delete[] tab;
        }
}

static int run_gat(char **v)
{
    const int dep = atoi(v[0]), esz = atoi(v[3]);
    const int64_t n = atoll(v[1]), nrow = atoll(v[2]);
    const int L_pp = (int)strlen(v[4]);
    if (strlen(v[5]) != (size_t)L_pp || L_pp > kMaxPattern) return 5;
    const uint64_t m1 = mask_of(v[4]), m2 = mask_of(v[5]), erase = strtoull(v[6], nullptr, 16);
    const char *why = pattern_check(m1, m2, L_pp);
    if (why) {
        fprintf(stderr, "%s\n", why);
        return 5;
    }
    const std::vector<uint8_t> xin = read_all(v[7]);
    if ((int64_t)xin.size() != n * nrow * esz) return 6;
    const int64_t n_out = dep ? depuncture_out_len(n, m1, L_pp) : puncture_out_len(n, m1, L_pp);
    GatherPlan g;
    gather_plan_make(m1, m2, L_pp, dep != 0, &g);
    Buf in((size_t)atoi(v[9]) * esz, xin.size(), xin.data()), out((size_t)atoi(v[10]) * esz, (size_t)(n_out * nrow * esz), nullptr);
    HostMem mem;
    mem.in = in.window();
    mem.in2 = Window{nullptr, nullptr};
    mem.out = out.window();
    switch (esz) {
    case 1: gather_rows<uint8_t>(mem, g, in.win(), out.win(), n, n_out, nrow, erase); break;
    case 2: gather_rows<uint16_t>(mem, g, in.win(), out.win(), n, n_out, nrow, erase); break;
    case 4: gather_rows<uint32_t>(mem, g, in.win(), out.win(), n, n_out, nrow, erase); break;
    case 8: gather_rows<uint64_t>(mem, g, in.win(), out.win(), n, n_out, nrow, erase); break;
    default: return 5;
    }
    out.guard_ok();
    write_all(v[8], out.win(), out.len);
    return 0;
}

static int run_cnt(char **v)
{
    const int64_t n = atoll(v[0]), nrow = atoll(v[1]), ts = atoll(v[2]), rs = atoll(v[3]);
    const int invert = atoi(v[4]);
    const std::vector<uint8_t> tx = read_all(v[5]), rx = read_all(v[6]);
    if (nrow < 1 || (int64_t)tx.size() != (nrow - 1) * ts + n || (int64_t)rx.size() != (nrow - 1) * rs + n) return 6;
    Buf bt(atoi(v[7]), tx.size(), tx.data()), br(atoi(v[8]), rx.size(), rx.data());
    HostMem mem;
    mem.in = bt.window();
    mem.in2 = br.window();
    mem.out = Window{nullptr, nullptr};
    const int64_t items = cnt_items_per_row(n);
    for (int64_t row = 0; row < nrow; ++row) {
        long long total = 0;   // the row's int64, integer adds in any order
        for (int64_t it = 0; it < items; ++it) {
            uint8_t *img_t = lds_alloc(kCntImgBytes), *img_r = lds_alloc(kCntImgBytes);
            const int64_t first = it * kCntWg;
            const int len = n - first < kCntWg ? (int)(n - first) : kCntWg;
            const uint8_t *gt = bt.win() + row * ts + first, *gr = br.win() + row * rs + first;
            for (int t = 0; t < kThreads; ++t) {
                blk::stage_in(mem, gt, len, img_t, t, kThreads);
                blk::stage_in(mem, gr, len, img_r, t, kThreads);
            }
            // ---- barrier
            for (int t = 0; t < kThreads; ++t) total += cnt_lane(img_t, blk::lead_of(gt), img_r, blk::lead_of(gr), len, 16 * t, invert);
            delete[] img_t;
            delete[] img_r;
        }
        printf("%lld%c", total, row + 1 == nrow ? '\n' : ' ');
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "plan" && argc == 2) {
        printf("run %d wg %d cnt_wg %d gather_item %d threads %d\n", kEncRun, kEncWg, kCntWg, kThreads * kGatherPerThread, kThreads);
        return 0;
    }
    if (cmd == "len" && argc == 6) {
        const int L_pp = (int)strlen(argv[4]);
        if (strlen(argv[5]) != (size_t)L_pp || L_pp > kMaxPattern) return 5;
        const uint64_t m1 = mask_of(argv[4]), m2 = mask_of(argv[5]);
        if (pattern_check(m1, m2, L_pp)) return 5;
        printf("%lld\n", (long long)(atoi(argv[2]) ? depuncture_out_len(atoll(argv[3]), m1, L_pp) : puncture_out_len(atoll(argv[3]), m1, L_pp)));
        return 0;
    }
    if (cmd == "enc" && argc == 12) return run_enc(argv + 2);
    if (cmd == "gat" && argc == 13) return run_gat(argv + 2);
    if (cmd == "cnt" && argc == 11) return run_cnt(argv + 2);
    return 2;
}
