// Host run of csrc/iir_route.hpp (standard headers only) over the recorded table tests/iir_routes/mi355x.txt (tools/record_iir_routes.py:
// every call's engines as the device noted them while the decision was still spread over iir_api.hip, iir_scan.hip and iir_par.hip).  The
// handles are made as iir_api.hip makes them (iir_design.hpp); the lazy facts come from iir_par_plan.hpp and iir_scan_plan.hpp.  The route of
// every row must name the recorded engines, ask no question twice, and -- hand-written cases -- use the buffers and helpers the names do not show.
//   g++ -O1 -std=c++17 -I scikit-dsp-comm_amd/csrc tests/host/iir_route_emul.cpp && ./a.out tests/iir_routes/mi355x.txt
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <fstream>
#include <string>
#include <tuple>
#include "iir_design.hpp"
#include "iir_route.hpp"

using namespace skdsp;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { ++g_fail; printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

// what iir_route.hpp reads of a handle, and what the queries cache on one
struct Handle {
    int dtype = 0, nsec = 0, order = 2;
    bool seq = false, unit = false;
    Handle *twin64 = nullptr;
    std::vector<Handle *> groups;
    int group_first = 0;
    std::vector<double> coef, A;
    int par_state = 0;
    ParExpansion pe;
    std::map<int, int> slot_K;
    int fstate[2] = {0, 0}, fnlv[2] = {0, 0};
    std::map<int64_t, ScanFacts> facts;
    ~Handle() { delete twin64; for (Handle *g : groups) delete g; }
};

// iir_api.hip: iir_create_common with the default options
static Handle *create(int nsec, const std::vector<double> &coef, int dtype, double seq_limit = 0.0)
{
    Handle *h = new Handle();
    h->dtype = dtype; h->nsec = nsec; h->coef = coef;
    if (nsec > 8) {
        const double spread = cascade_spread(coef.data(), nsec);
        const double limit = seq_limit > 0.0 ? seq_limit : iir_dbl(dtype) ? 2.5e-13 : 2.5e-9;
        if (!(spread <= limit)) { h->seq = true; return h; }
    }
    bool grouped = nsec > 8;
    if (grouped && !iir_dbl(dtype) && !(boundary_cost(coef.data(), nsec) <= 16.0)) {
        if (nsec > 12) {
            h->twin64 = create(nsec, coef, dtype == kIirC64 ? kIirC128 : kIirF64, 2.5e-9);
            return h;
        }
        grouped = false;
    }
    if (grouped) {
        int s0 = 0;
        for (const int cnt : group_sizes(nsec, 8)) {
            Handle *g = create(cnt, std::vector<double>(coef.begin() + 5 * s0, coef.begin() + 5 * (s0 + cnt)), dtype);
            g->group_first = s0;
            h->groups.push_back(g);
            s0 += cnt;
        }
        return h;
    }
    std::vector<double> scale;
    h->unit = unit_tail(h->coef.data(), nsec, scale);
    return h;
}

struct Queries {
    ParOptions po{1, 1, 1, 1, 1};
    std::set<std::tuple<Handle *, int, int64_t, int, int, int>> asked;   // per call: no question twice
    int repeats = 0;
    void note(Handle *h, int what, int64_t a, int b = 0, int c = 0, int d = 0)
    {
        if (!asked.insert(std::make_tuple(h, what, a, b, c, d)).second) ++repeats;
    }
    ParChoice par(Handle *h, bool il, int nrow, int dec, int up, int64_t n)
    {
        note(h, il ? 1 : 0, n, nrow, dec, up);
        ParChoice no;
        if (h->order != 2 || !par_call_shape_ok(h->nsec, il, nrow, dec, up, n)) return no;
        if (!h->par_state) h->par_state = par_expand(h->coef.data(), h->nsec, h->pe) ? 1 : -1;
        if (h->par_state != 1) return no;
        return par_choose(h->nsec, iir_dbl(h->dtype), il, nrow, dec, up, n, po, [&](int slot) {
            if (!h->slot_K.count(slot)) {
                const ParTableValues v = par_table_values(h->pe, par_slot_T(slot), par_slot_chunks(slot), par_slot_negl(slot), par_slot_dbl(slot) ? 8 : 4);   // (iir_par.hip: par_max_k)
                h->slot_K[slot] = v.failed ? 0 : v.K;
            }
            return h->slot_K[slot];
        });
    }
    int fused_cached(Handle *h, bool il, int &fstate, int &fnlv)
    {
        fstate = h->fstate[il]; fnlv = h->fnlv[il];
        return 0;
    }
    void fused_remember(Handle *h, bool il, int fstate, int fnlv) { h->fstate[il] = fstate; h->fnlv[il] = fnlv; }
    int scan_facts(Handle *h, int64_t T, ScanFacts &f)
    {
        if (h->A.empty()) h->A = scan_A_host(h->coef.data(), h->nsec, h->order);
        note(h, 2, T);
        if (!h->facts.count(T)) {
            const ScanTables t = scan_tables(h->coef.data(), h->nsec, h->order, h->A, T, iir_dbl(h->dtype));
            h->facts[T] = ScanFacts{t.n_lv, t.n_lb, t.gt_T};
        }
        f = h->facts[T];
        return 0;
    }
};

// skdsp_debug_path's list for a route: runtime.hip's note_path drops an engine that repeats the one before it
static std::string engines_of(const IirRoute<Handle> &r, const IirCall &c)
{
    std::vector<std::string> names;
    auto note = [&](const std::string &e) { if (names.empty() || names.back() != e) names.push_back(e); };
    for (size_t i = 0; i < r.steps.size();) {
        const size_t block = r.steps[i].block > 0 ? r.steps[i].block : 1;
        for (int64_t row = 0; row < (r.steps[i].block > 0 ? c.nrow : 1); ++row)
            for (size_t j = i; j < i + block; ++j) {
                const IirStep<Handle> &s = r.steps[j];
                if (s.engine == kEngSeq) note("iir_seq");
                if (s.engine == kEngFused) note("iir_fused");
                if (s.engine == kEngScan) note("iir_scan");
                if (s.engine == kEngPar) {
                    note("iir_par");
                    if (s.par.v32_wanted && par_v32_probe(s.h->pe, par_slot_T(s.par.slot), kParV32Limit) <= kParV32Limit) note("iir_par_v32");
                }
            }
        i += block;
    }
    std::string out;
    for (const std::string &e : names) out += (out.empty() ? "" : ",") + e;
    return out.empty() ? "-" : out;
}

static IirRouteOptions options_of(const std::string &text)
{
    IirRouteOptions o;
    if (text == "-") return o;
    std::stringstream ss(text);
    std::string kv;
    while (std::getline(ss, kv, ',')) {
        const std::string k = kv.substr(0, kv.find('='));
        const int v = atoi(kv.substr(kv.find('=') + 1).c_str());
        if (k == "iir_par") o.iir_par = v;
        else if (k == "iir_planar") o.iir_planar = v;
        else if (k == "iir_up_fused") o.iir_up_fused = v;
        else if (k == "iir_dn_full") o.iir_dn_full = v;
        else if (k == "iir_two_pass") o.iir_two_pass = v;
        else if (k == "iir_no_mfma") o.iir_no_mfma = v;
        else { ++g_fail; printf("FAIL unknown option %s\n", k.c_str()); }
    }
    return o;
}

static IirCall call_of(const std::string &call, int arg, int64_t n, int cus)
{
    IirCall c;
    c.kind = call == "up" ? kIirUp : call == "dn" ? kIirDn : call == "rows" ? kIirRows : kIirFilter;
    c.n = n; c.rate = arg; c.num_cus = cus;
    if (call == "rows") { c.nrow = 3; c.x_stride = c.y_stride = n + 7; }
    c.zi = c.zf = call == "state";
    return c;
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: iir_route_emul TABLE\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int cus = 0, rows = 0;
    std::map<std::string, std::pair<int, std::vector<double>>> designs;
    std::map<std::pair<int, std::string>, std::unique_ptr<Handle>> handles;
    auto handle_of = [&](int dtype, const std::string &name) {
        std::unique_ptr<Handle> &h = handles[{dtype, name}];
        if (!h) h.reset(create(designs.at(name).first, designs.at(name).second, dtype));
        return h.get();
    };
    std::set<std::string> lists;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        if (line.rfind("# cus=", 0) == 0) { cus = atoi(line.c_str() + 6); continue; }
        if (line.rfind("# design ", 0) == 0) {
            std::string hash, word, name;
            int nsec;
            ss >> hash >> word >> name >> nsec;
            std::vector<double> sos(6 * nsec), coef;
            for (double &v : sos) ss >> v;
            EXPECT(sos_rows_to_coef(sos.data(), nsec, coef));
            designs[name] = {nsec, coef};
            continue;
        }
        if (line.empty() || line[0] == '#') continue;
        int dtype, arg, rc;
        int64_t n;
        std::string design, call, opts, engines;
        ss >> dtype >> design >> call >> arg >> n >> opts >> rc >> engines;
        Queries q;
        const IirCall c = call_of(call, arg, n, cus);
        const IirRoute<Handle> r = iir_route(handle_of(dtype, design), c, options_of(opts), q);
        const std::string got = r.status ? "status " + std::to_string(r.status) : engines_of(r, c);
        ++rows;
        lists.insert(engines);
        if (rc != 0 || got != engines || q.repeats) {
            ++g_fail;
            printf("FAIL %s\n  route: %s, %d question(s) asked twice\n", line.c_str(), got.c_str(), q.repeats);
        }
    }
    EXPECT(cus > 0 && rows > 300 && lists.size() >= 6);

    // what the engine names do not show
    auto route = [&](int dtype, const char *design, const char *call, int arg, int64_t n, const char *opts) {
        Queries q;
        return iir_route(handle_of(dtype, design), call_of(call, arg, n, cus), options_of(opts), q);
    };
    {   // complex through two planes: split into workspace slot 3, both planes in one launch in place, interleave into y
        const IirRoute<Handle> r = route(kIirC64, "e8", "filter", 1, 1000, "iir_planar=1");
        EXPECT(r.steps.size() == 3 && r.steps[0].engine == kEngDeinterleave && r.steps[0].src.kind == kBufX && r.steps[0].dst.kind == kBufPlanes &&
               r.steps[0].dst.bytes == 2 * 1024 * 4 && r.steps[1].engine == kEngPar && r.steps[1].nrow == 2 && r.steps[1].x_stride == 1024 &&
               r.steps[1].src == r.steps[1].dst && !r.steps[1].interleaved && r.steps[2].engine == kEngInterleave && r.steps[2].dst.kind == kBufY);
    }
    {   // interleaved: one launch on the caller's buffers
        const IirRoute<Handle> r = route(kIirC64, "e8", "filter", 1, 1000, "-");
        EXPECT(r.steps.size() == 1 && r.steps[0].engine == kEngPar && r.steps[0].interleaved && r.steps[0].nrow == 1 && r.steps[0].src.kind == kBufX && r.steps[0].dst.kind == kBufY);
    }
    {   // .up: fused into the parallel form, or zero-stuff into y and filter y in place; complex: zero-stuff into the planes
        IirRoute<Handle> r = route(kIirF32, "e8", "up", 3, 1000, "-");
        EXPECT(r.steps.size() == 1 && r.steps[0].engine == kEngPar && r.steps[0].up == 3 && r.steps[0].n == 3000);
        r = route(kIirF32, "e8", "up", 3, 1000, "iir_up_fused=0");
        EXPECT(r.steps.size() == 2 && r.steps[0].engine == kEngZeroStuff && r.steps[0].up == 3 && r.steps[0].n == 1000 && r.steps[0].dst.kind == kBufY &&
               r.steps[1].src.kind == kBufY && r.steps[1].dst.kind == kBufY && r.steps[1].n == 3000 && r.steps[1].up == 1);
        r = route(kIirC128, "e8", "up", 3, 1000, "iir_up_fused=0");
        EXPECT(r.steps.size() == 3 && r.steps[0].engine == kEngZeroStuffPlanes && r.steps[0].dst.bytes == 2 * 3008 * 8 && r.steps[1].nrow == 2 && r.steps[2].n == 3000);
    }
    {   // .dn: the engines' decimating store up to 4096, else the full-rate result in workspace slot 2 and a strided copy
        IirRoute<Handle> r = route(kIirF32, "e8", "dn", 96, 1000, "-");
        EXPECT(r.steps.size() == 1 && r.steps[0].dec == 96 && r.steps[0].dst.kind == kBufY);
        r = route(kIirC64, "e8", "dn", 4097, 12291, "-");
        EXPECT(r.steps.size() == 2 && r.steps[0].dst.kind == kBufFull && r.steps[0].dst.bytes == 12291 * 8 + 256 && r.steps[0].dec == 1 &&
               r.steps[1].engine == kEngDownsample && r.steps[1].dec == 4097 && r.steps[1].src.kind == kBufFull);
        r = route(kIirF32, "e8", "dn", 3, 1000, "iir_dn_full=1");
        EXPECT(r.steps.size() == 2 && r.steps[1].engine == kEngDownsample);
    }
    {   // groups: in place behind the first; a decimating call keeps the full-rate signal in the handle's buffer; states by section
        IirRoute<Handle> r = route(kIirF64, "b16", "state", 1, 1000, "-");
        EXPECT(r.steps.size() == 2 && r.steps[0].src.kind == kBufX && r.steps[0].dst.kind == kBufY && r.steps[1].src.kind == kBufY && r.steps[0].zi && r.steps[1].zf &&
               r.steps[0].state_first == 0 && r.steps[1].state_first == 8 && r.steps[0].state_D == 32 && r.steps[1].state_D == 32);
        r = route(kIirF64, "b16", "dn", 3, 1000, "-");
        EXPECT(r.steps.size() == 2 && r.steps[0].dst.kind == kBufGroupTmp && r.steps[0].dst.bytes == 1000 * 8 + 256 && r.steps[0].dec == 1 &&
               r.steps[1].src.kind == kBufGroupTmp && r.steps[1].dst.kind == kBufY && r.steps[1].dec == 3);
    }
    {   // the float64 twin: widen into the handle's buffer, the twin's groups in place there, narrow into y; .dn: the kept outputs apart
        IirRoute<Handle> r = route(kIirF32, "c13", "filter", 1, 1000, "-");
        Handle *h = handle_of(kIirF32, "c13");
        EXPECT(h->twin64 && h->twin64->groups.size() == 2);
        EXPECT(r.steps.size() == 4 && r.steps[0].engine == kEngWiden && r.steps[0].dst.kind == kBufTwinIn && r.steps[0].dst.owner == h &&
               r.steps[1].h == h->twin64->groups[0] && r.steps[1].src.kind == kBufTwinIn && r.steps[2].dst.kind == kBufTwinIn &&
               r.steps[3].engine == kEngNarrow && r.steps[3].src.kind == kBufTwinIn && r.steps[3].dst.kind == kBufY && r.steps[3].n == 1000);
        r = route(kIirF32, "c13", "dn", 2, 1000, "-");
        EXPECT(r.steps.size() == 4 && r.steps[1].dst.kind == kBufGroupTmp && r.steps[1].dst.owner == h->twin64 && r.steps[2].dst.kind == kBufTwinOut &&
               r.steps[3].src.kind == kBufTwinOut && r.steps[3].n == 500);
    }
    {   // rows: one launch where the parallel form takes them, else a block of steps per row
        IirRoute<Handle> r = route(kIirF32, "e8", "rows", 1, 1000, "-");
        EXPECT(r.steps.size() == 1 && r.steps[0].nrow == 3 && r.steps[0].x_stride == 1007 && r.steps[0].block == 0);
        r = route(kIirC64, "rep2", "rows", 1, 1000, "-");
        EXPECT(!r.steps.empty() && r.steps[0].block == (int)r.steps.size());
        r = route(kIirF64, "c20", "rows", 1, 1000, "-");
        EXPECT(r.steps.size() == 1 && r.steps[0].engine == kEngSeq && r.steps[0].nrow == 3);
    }
    {   // the two-pass scan: geometry and mode decided with the route
        const int64_t n = (int64_t)96 * 512 * 256 + 1;
        IirRoute<Handle> r = route(kIirC64, "b2", "filter", 1, n, "iir_par=0,iir_two_pass=1");
        EXPECT(r.steps.size() == 1 && r.steps[0].engine == kEngScan && r.steps[0].interleaved && r.steps[0].fast && r.steps[0].geom.T == 128);
        r = route(kIirC64, "b2", "filter", 1, n - 1, "iir_par=0,iir_two_pass=1");
        EXPECT(r.steps.size() == 3 && r.steps[1].engine == kEngScan && !r.steps[1].interleaved && !r.steps[1].fast && r.steps[1].geom.T == 96 && r.steps[1].nrow == 2);
    }
    printf(g_fail ? "%d FAILED\n" : "%d rows OK\n", g_fail ? g_fail : rows);
    return g_fail ? 1 : 0;
}
