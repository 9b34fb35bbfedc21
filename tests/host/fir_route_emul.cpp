// Host run of csrc/fir_route.hpp (standard headers only: no device toolchain): the FIR routing decision against the table recorded on the device
// before the decision was gathered into that header (tests/fir_routes/mi355x.txt, tools/record_fir_routes.py), and hand-written cases for what the
// engine names of the table cannot show.  The "parent" of the comments is the commit the table's header names; its fir_api.hip held the decision.
//   fir_route_emul <table>
#include "fir_route.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

using namespace skdsp;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++failures;                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

static bool set_option(FirRouteOptions &o, const std::string &name, int v)
{
#define OPT(f) if (name == #f) { o.f = v; return true; }
    OPT(fir_algo) OPT(dn_no_ols) OPT(fir_mm) OPT(fir_bx) OPT(fir_up_ols_min) OPT(fir_up_rows_min) OPT(fir_up_pair) OPT(fir_up4k) OPT(fir_up2k)
    OPT(fir_up_rep) OPT(fir_dn_fold) OPT(fir_dn4k) OPT(fir_updn_fused)
#undef OPT
    return false;
}

static std::string join(const std::vector<std::string> &v)
{
    std::string s;
    for (const std::string &e : v) s += (s.empty() ? "" : ",") + e;
    return s.empty() ? "-" : s;
}

// does the execution of r end in a refusal?  (a tap-segment call: one of its segments)
static bool refuses(const FirRoute &r, FirShape h, const FirCall &c, const FirRouteOptions &o)
{
    if (r.engine == kRouteRefused) return true;
    if (r.seg == 0) return false;
    if (r.head) h.ntaps = r.head;
    const int64_t n = c.L == 1 ? (c.n / c.M) * c.M : c.n;
    for (int si = 0; si < fir_parts_count(h, r.seg); ++si) {
        FirSegment s;
        if (!fir_parts_segment(h, r.seg, si, n, c.n_hist, c.L, c.M, &s)) break;
        const FirShape p{h.dtype, s.taps, h.taps_complex, h.algo};
        const FirCall cs{s.n, s.n_hist, c.L, c.M, c.L == 1 && c.M == 1, si == 0 ? c.y_low : 0u, false, c.num_cus};
        const int runs = fir_up_model_runs();
        const FirRoute rs = fir_route_single(p, cs, o);
        CHECK(fir_up_model_runs() - runs <= 1, "the cost model ran %d times for one segment", fir_up_model_runs() - runs);
        CHECK(rs.seg == 0, "a segment of %d taps is cut again", s.taps);
        if (rs.engine == kRouteRefused) return true;
    }
    return false;
}

static int check_table(const char *path)
{
    std::ifstream f(path);
    if (!f) { std::printf("cannot open %s\n", path); return -1; }
    std::string line;
    int cus = 0, rows = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        if (line[0] == '#') {
            const size_t at = line.find("cus=");
            if (at != std::string::npos) cus = std::atoi(line.c_str() + at + 4);
            continue;
        }
        CHECK(cus > 0, "no CU count in the header of %s", path);
        if (cus <= 0) return -1;
        std::istringstream in(line);
        int dtype, tc, algo, ntaps, L, M, rc;
        long long n, n_hist, y_off;
        std::string opts, engines, crc;
        in >> dtype >> tc >> algo >> ntaps >> L >> M >> n >> n_hist >> y_off >> opts >> rc >> engines >> crc;
        CHECK(!in.fail(), "bad row: %s", line.c_str());
        if (in.fail()) continue;
        FirRouteOptions o;
        if (opts != "-") {
            std::istringstream os(opts);
            std::string kv;
            while (std::getline(os, kv, ',')) {
                const size_t eq = kv.find('=');
                CHECK(eq != std::string::npos && set_option(o, kv.substr(0, eq), std::atoi(kv.c_str() + eq + 1)), "unknown option in: %s", line.c_str());
            }
        }
        const FirShape h{dtype, ntaps, tc != 0, algo};
        // (the recorder's y is a 256-byte aligned buffer plus y_off elements)
        const FirCall c{n, n_hist, L, M, L == 1 && M == 1, (unsigned)((y_off * fir_esz(h)) & 255), true, cus};
        const int runs = fir_up_model_runs();
        const FirRoute r = fir_route(h, c, o);
        CHECK(fir_up_model_runs() - runs <= 1, "the cost model ran %d times: %s", fir_up_model_runs() - runs, line.c_str());
        const std::string got = join(fir_route_engines(r, h, c, o));
        CHECK(got == engines, "engines %s, recorded %s: %s", got.c_str(), engines.c_str(), line.c_str());
        CHECK(refuses(r, h, c, o) == (rc != 0), "refusal %d, recorded rc %d: %s", (int)refuses(r, h, c, o), rc, line.c_str());
        ++rows;
    }
    std::printf("%d rows of %s checked (%d CUs)\n", rows, path, cus);
    CHECK(rows > 0, "empty table");
    return rows;
}

static void hand_cases()
{
    const int cus = 256;
    const int64_t n = 1 << 20;
    FirRouteOptions walk_only;   // the walk wherever it applies: no tile interpolators, no cost model
    walk_only.fir_up4k = 0; walk_only.fir_up_rep = 0; walk_only.fir_up_ols_min = -2;
    auto up = [&](int dtype, int ntaps, int L, unsigned y_low, const FirRouteOptions &o, bool scratch_free = true) {
        return fir_route(FirShape{dtype, ntaps, false, kFirAuto}, FirCall{n, 0, L, 1, false, y_low, scratch_free, cus}, o);
    };
    // 1. float32, even L, an 8-byte aligned y: phases in pairs (parent fir_api.hip:363, fir_ols.hip:1199); fewer than 7 pairs stay strided (:202, :364)
    FirRoute r = up(kFirF32, 1024, 4, 0, walk_only);
    CHECK(r.engine == kRouteWalk && r.paired && !r.rows && r.dec == 1 && r.copy == kCopyNone, "f32 L=4: engine %d paired %d rows %d", r.engine, r.paired, r.rows);
    // 2. ... y 4 bytes off: no pairs, and float32 rows start at L = 9 (:205)
    r = up(kFirF32, 1024, 4, 4, walk_only);
    CHECK(r.engine == kRouteWalk && !r.paired && !r.rows, "f32 L=4 odd y: paired %d rows %d", r.paired, r.rows);
    // 3. 8 pairs: rows of pairs, woven out of workspace slot 2 (:202, :368-378)
    r = up(kFirF32, 1024, 16, 0, walk_only);
    CHECK(r.paired && r.rows && r.copy == kCopyWeave && r.slot == 2, "f32 L=16: paired %d rows %d copy %d slot %d", r.paired, r.rows, r.copy, r.slot);
    // 4. L = 2 is one pair, one row: nothing to weave, whatever the option asks (:364)
    FirRouteOptions rows2 = walk_only;
    rows2.fir_up_rows_min = 2;
    r = up(kFirF32, 1024, 2, 0, rows2);
    CHECK(r.paired && !r.rows && r.copy == kCopyNone, "f32 L=2: paired %d rows %d", r.paired, r.rows);
    // 5. odd L in 7 .. 13: pairs in the strided form at a 4-byte aligned y (fir_ols.hip:1200, fir_api.hip:365-367); 15 and 5: single phases, rows from 9 on
    for (int L : {7, 9, 11, 13}) {
        r = up(kFirF32, 2048, L, 4, walk_only);
        CHECK(r.engine == kRouteWalk && r.paired && !r.rows, "f32 L=%d: paired %d rows %d", L, r.paired, r.rows);
    }
    r = up(kFirF32, 2048, 15, 4, walk_only);
    CHECK(!r.paired && r.rows && r.copy == kCopyWeave, "f32 L=15: paired %d rows %d", r.paired, r.rows);
    r = up(kFirF32, 2048, 5, 4, walk_only);
    CHECK(!r.paired && !r.rows, "f32 L=5: paired %d rows %d", r.paired, r.rows);
    // 6. ... rows asked for by option win over the pairs of an odd L (:366)
    FirRouteOptions rows4 = walk_only;
    rows4.fir_up_rows_min = 4;
    r = up(kFirF32, 2048, 9, 4, rows4);
    CHECK(!r.paired && r.rows && r.copy == kCopyWeave, "f32 L=9 rows_min=4: paired %d rows %d", r.paired, r.rows);
    // 7. rows from L = 7 (complex64), 9 (float32), 6 (float64), never complex128 (:204-209); float64 pairs need a 16-byte aligned y and never leave as rows (:202, fir_ols64.hip:689)
    CHECK(up(kFirC64, 2048, 7, 0, walk_only).rows && !up(kFirC64, 2048, 6, 0, walk_only).rows, "c64 rows from L = 7");
    CHECK(up(kFirF32, 2048, 9, 2, walk_only).rows && !up(kFirF32, 2048, 8, 4, walk_only).rows, "f32 rows from L = 9");
    CHECK(up(kFirF64, 1024, 6, 8, walk_only).rows && !up(kFirF64, 1024, 5, 8, walk_only).rows, "f64 rows from L = 6");
    CHECK(up(kFirF64, 1024, 6, 8, walk_only).engine == kRouteWalk64 && !up(kFirF64, 1024, 6, 8, walk_only).paired, "f64 L=6, y 8 bytes off: no pairs");
    r = up(kFirF64, 1024, 6, 16, walk_only);
    CHECK(r.paired && !r.rows, "f64 L=6 aligned: paired %d rows %d", r.paired, r.rows);
    CHECK(!up(kFirC128, 1024, 24, 0, walk_only).rows, "c128 never rows");
    // 8. inside a tap-segment call workspace slot 2 is taken: no rows (:364)
    CHECK(!up(kFirC64, 2048, 7, 0, walk_only, false).rows, "no rows without scratch");
    // 9. L / M through the walk: its store keeps every M-th (dec = M, :383); option fir_updn_fused = 0: out of scratch (:384-388), and not at all
    //    inside a tap-segment call (:382)
    auto updn = [&](const FirRouteOptions &o, bool scratch_free) {
        return fir_route(FirShape{kFirC64, 3072, false, kFirAuto}, FirCall{n, 0, 3, 2, false, 0, scratch_free, cus}, o);
    };
    r = updn(walk_only, true);
    CHECK(r.engine == kRouteWalk && r.dec == 2 && r.copy == kCopyNone, "3/2 fused: engine %d dec %d copy %d", r.engine, r.dec, r.copy);
    FirRouteOptions unfused = walk_only;
    unfused.fir_updn_fused = 0;
    r = updn(unfused, true);
    CHECK(r.engine == kRouteWalk && r.dec == 1 && r.copy == kCopyEveryMth && r.slot == 2, "3/2 unfused: engine %d dec %d copy %d", r.engine, r.dec, r.copy);
    r = updn(unfused, false);
    CHECK(r.engine != kRouteWalk && r.copy == kCopyNone, "3/2 unfused without scratch: engine %d", r.engine);
    // 10. the full-rate fallback of .dn: workspace slot 2, slot 3 inside a tap-segment call (:142, :150, :185); float32 takes the decimating store up to M = 32768 (:184)
    const FirRouteOptions dflt;
    auto dn = [&](int dtype, int M, bool scratch_free, const FirRouteOptions &o) {
        return fir_route_single(FirShape{dtype, 400, false, kFirAuto}, FirCall{(int64_t)1 << 17, 0, 1, M, false, 0, scratch_free, cus}, o);
    };
    r = dn(kFirC64, 40000, true, dflt);
    CHECK(r.copy == kCopyFullRate && r.slot == 2 && r.direct_refused && r.M == 40000 && r.dec == 1, "c64 M=40000: copy %d slot %d", r.copy, r.slot);
    CHECK(r.engine == kRouteOls, "... its full-rate filter of 400 taps is overlap-save: %d", r.engine);
    r = dn(kFirC64, 40000, false, dflt);
    CHECK(r.copy == kCopyFullRate && r.slot == 3, "c64 M=40000 in a segment: copy %d slot %d", r.copy, r.slot);
    r = dn(kFirC64, 20000, false, dflt);
    CHECK(r.engine == kRouteOls && r.dec == 20000 && r.copy == kCopyNone && r.direct_refused, "c64 M=20000: engine %d dec %d", r.engine, r.dec);
    FirRouteOptions no_ols;
    no_ols.dn_no_ols = 1;
    r = dn(kFirF64, 5000, false, no_ols);
    CHECK(r.copy == kCopyFullRate && r.slot == 3, "f64 M=5000 dn_no_ols in a segment: copy %d slot %d", r.copy, r.slot);
    r = dn(kFirF64, 5000, true, dflt);
    CHECK(r.engine == kRouteOls64 && r.dec == 5000 && r.copy == kCopyNone, "f64 M=5000: engine %d dec %d", r.engine, r.dec);
    // 11. segments: a multiple of lcm(L, M), at most 4096 (float64: 2048) taps per phase (:72-73)
    const FirShape f32{kFirF32, 100000, false, kFirAuto}, f64{kFirF64, 100000, false, kFirAuto};
    CHECK(fir_parts_seg(f32, 1, 1) == 4096 && fir_parts_seg(f64, 1, 1) == 2048, "seg of .filter");
    CHECK(fir_parts_seg(f32, 1, 3) == 4095 && fir_parts_seg(f32, 3, 2) == 12288 && fir_parts_seg(f32, 7, 4) == 28672, "seg of 1/3, 3/2, 7/4");
    CHECK(fir_parts_seg(f32, 5000, 3) == 1365 * 15000 && fir_parts_seg(f32, 1, 5000) == 5000, "seg of 5000/3, 1/5000");
    for (int L : {1, 2, 3, 7, 12, 16})
        for (int M : {1, 2, 3, 5, 12, 100}) {
            const int seg = fir_parts_seg(f64, L, M), lcm = L / std::gcd(L, M) * M;
            CHECK(seg % lcm == 0 && seg >= lcm && (seg / L <= 2048 || seg == lcm), "seg %d of %d/%d", seg, L, M);
        }
    r = fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 0, 1, 3, false, 0, true, cus}, dflt);
    CHECK(r.engine == kRouteParts && r.seg == 4095, ".dn by 3 of 12288 taps: engine %d seg %d", r.engine, r.seg);
    // ... one output period longer than a launch takes: refused (the parent cut its one segment again, without end: :73, :143)
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 0, 1, 20000, false, 0, true, cus}, dflt).engine == kRouteRefused, ".dn by 20000 of 12288 taps");
    CHECK(fir_route(FirShape{kFirF64, 12288, false, kFirAuto}, FirCall{n, 0, 1, 4000, false, 0, true, cus}, dflt).engine == kRouteRefused, "float64 .dn by 4000 of 12288 taps");
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 0, 1, 4000, false, 0, true, cus}, dflt).engine == kRouteParts, ".dn by 4000 of 12288 taps");
    // ... a partial history must be whole output periods (:87)
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 301, 1, 3, false, 0, true, cus}, dflt).engine == kRouteRefused, "n_hist = 301 of .dn by 3");
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 300, 1, 3, false, 0, true, cus}, dflt).engine == kRouteParts, "n_hist = 300 of .dn by 3");
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{n, 12285, 1, 3, false, 0, true, cus}, dflt).engine == kRouteParts, "a complete history of .dn by 3");
    // 12. heads: the next power of two >= n, below the tap count, from rest and for .filter only (:405-408, :420)
    CHECK(fir_head_taps(1024, 100) == 128 && fir_head_taps(1024, 512) == 512 && fir_head_taps(1024, 513) == 0 && fir_head_taps(1024, 1) == 1, "heads of 1024 taps");
    CHECK(fir_head_taps(1024, 0) == 0 && fir_head_taps(100, 100) == 0 && fir_head_taps(100, 64) == 64 && fir_head_taps(100, 65) == 0, "heads at the edges");
    const FirShape lp{kFirC64, 1024, false, kFirAuto};
    CHECK(fir_route(lp, FirCall{100, 0, 1, 1, true, 0, true, cus}, dflt).head == 128, "head of a .filter call from rest");
    CHECK(fir_route(lp, FirCall{100, 5, 1, 1, true, 0, true, cus}, dflt).head == 0, "no head behind a history");
    CHECK(fir_route(lp, FirCall{100, 0, 1, 1, false, 0, true, cus}, dflt).head == 0, "no head for the rate changers");
    CHECK(fir_route(FirShape{kFirF32, 12288, false, kFirAuto}, FirCall{5000, 0, 1, 1, true, 0, true, cus}, dflt).seg == 4096, "a head of 8192 taps runs as segments");
    // 13. one evaluation of the cost model for a call that consulted it three times (:352, :359, :362)
    const int runs = fir_up_model_runs();
    r = fir_route(FirShape{kFirC64, 1024, false, kFirAuto}, FirCall{12289, 0, 4, 1, false, 0, true, cus}, dflt);
    CHECK(fir_up_model_runs() - runs == 1, "complex64, 1024 taps, L = 4: %d evaluations", fir_up_model_runs() - runs);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: %s <table>\n", argv[0]); return 2; }
    hand_cases();
    if (check_table(argv[1]) <= 0) return 1;
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
