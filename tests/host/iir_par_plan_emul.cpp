// Host run of the parallel-form IIR plan code (no GPU): csrc/iir_par_plan.hpp and standard headers only -- that this file compiles is
// itself the check that the expansion, the V32 probe, the table values and the dispatch decision need no device.  Inputs are powers of
// two (or sums of a few), so every comparison is exact unless it says otherwise.
// Build: g++ -O1 -std=c++17 -I scikit-dsp-comm_amd/csrc tests/host/iir_par_plan_emul.cpp -o /tmp/iir_par_plan_emul
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "iir_par_plan.hpp"

using namespace skdsp;

static int g_fail = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            ++g_fail;                                                  \
        }                                                              \
    } while (0)

static const ParOptions kDefaults{1, 1, 1, 1, 1};   // iir_dn_t96, iir_up_jump, iir_up_lean, iir_dn_compact, iir_par_v32

// par_choose with a K query that answers k96 for the 96-sample slots and 1 for the others, and records which slots were asked
struct Asked { std::vector<int> slots; };
static ParChoice choose(int nsec, bool dbl, bool il, int nrow, int dec, int up, int64_t n, const ParOptions &o = kDefaults, int k96 = 1, Asked *asked = nullptr)
{
    return par_choose(nsec, dbl, il, nrow, dec, up, n, o, [&](int slot) {
        if (asked) asked->slots.push_back(slot);
        return slot >= 4 ? k96 : 1;
    });
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // ---- par_expand
    {   // 1 / (1 - 0.5 q): one real pole, no direct term
        const double c[5] = {1.0, 0.0, 0.0, -0.5, 0.0};
        ParExpansion P;
        EXPECT(par_expand(c, 1, P));
        EXPECT(P.nsec == 1 && P.c0 == 0.0L && P.r0[0] == 1.0L && P.r1[0] == 0.0L);
        EXPECT(P.gamma == 1.0 && P.al[0] == 0.5 && P.be[0] == 0.0 && P.na1[0] == 0.5 && P.na2[0] == 0.0);
        EXPECT(P.ir_err == 0.0 && P.kappa == 1.0 && P.l1h == 2.0);
    }
    {   // 1 / ((1 - 0.5 q)(1 - 0.25 q)) = 2 / (1 - 0.5 q) - 1 / (1 - 0.25 q)
        const double c[10] = {1.0, 0.0, 0.0, -0.5, 0.0, 1.0, 0.0, 0.0, -0.25, 0.0};
        ParExpansion P;
        EXPECT(par_expand(c, 2, P));
        EXPECT(P.r0[0] == 2.0L && P.r0[1] == -1.0L && P.r1[0] == 0.0L && P.r1[1] == 0.0L && P.c0 == 0.0L && P.gamma == 1.0);
        EXPECT(P.al[0] == 1.0 && P.al[1] == -0.25);
    }
    {   // refusals
        ParExpansion P;
        const double twice[10] = {1.0, 0.0, 0.0, -0.5, 0.25, 1.0, 0.0, 0.0, -0.5, 0.25};   // two sections sharing a pole pair
        EXPECT(!par_expand(twice, 2, P));
        const double heavy[10] = {1.0, 0.5, 0.25, 0.0, 0.0, 1.0, 0.0, 0.0, -0.5, 0.0};     // numerator degree 2, denominator degree 1
        EXPECT(!par_expand(heavy, 2, P));
        const double bad[5] = {1.0, nan, 0.0, -0.5, 0.0};
        EXPECT(!par_expand(bad, 1, P));
    }

    // ---- par_table_values: poles 0.5 and 0.25, g_k[i] = p_k^i
    ParExpansion two;
    {
        const double c[10] = {1.0, 0.0, 0.0, -0.5, 0.0, 1.0, 0.0, 0.0, -0.25, 0.0};
        EXPECT(par_expand(c, 2, two));
    }
    for (int T : {128, 96}) {
        const ParTableValues v = par_table_values(two, T, 64, 1e-18L, 4);
        EXPECT(!v.failed && v.n_lv == 0 && v.K == 1);
        EXPECT(v.gt.size() == (size_t)T * 16 && v.lvl.size() == (size_t)6 * 2 * 4 && v.psi.size() == (size_t)7 * 2 * 4);
        bool layout = true;
        for (int t = 0; t < T; ++t)
            for (int k = 0; k < 2; ++k) {
                const size_t at = (size_t)(t / 4) * 64 + (size_t)(t % 4) * 16 + 2 * k;
                const int sh = k == 0 ? 1 : 2;   // p_k = 2^-sh
                layout = layout && v.gt[at] == std::ldexp(1.0, -sh * (T - 1 - t)) && v.gt[at + 1] == (t == T - 1 ? 0.0 : std::ldexp(1.0, -sh * (T - 2 - t)));
            }
        EXPECT(layout);
        // Phi = [p^T, 0; p^(T-1), 0]; level l holds its 2^l-th power [p^(T 2^l), 0; p^(T 2^l - 1), 0] (zero once it underflows a double)
        for (int l = 0; l < 6; ++l) {
            const double *m = v.lvl.data() + ((size_t)l * 2 + 0) * 4;
            EXPECT(m[0] == std::ldexp(1.0, -(T << l)) && m[1] == 0.0 && m[2] == std::ldexp(1.0, -(T << l) + 1) && m[3] == 0.0);
            EXPECT(m[0] == (l == 0 ? v.lvl[0] : std::pow(v.lvl[0], (double)(1 << l))));
        }
    }
    {   // a pole at 0.9995 remembers more than four 8192-sample segments (0.9995^32768 = 8e-8)
        const double c[5] = {1.0, 0.0, 0.0, -0.9995, 0.0};
        ParExpansion P;
        EXPECT(par_expand(c, 1, P));
        const ParTableValues v = par_table_values(P, 128, 64, 1e-18L, 4);
        EXPECT(v.failed && v.K == 0);
    }
    {   // the resonator of tools/ab_dispatch.py (pole radius 0.997 at angle 0.6) looks back over more than one float32 segment at both chunk lengths
        const double r = 0.997, c[5] = {1.0, 0.0, 0.0, -2.0 * r * std::cos(0.6), r * r};
        ParExpansion P;
        EXPECT(par_expand(c, 1, P));
        const ParTableValues v128 = par_table_values(P, 128, 64, 1e-18L, 4), v96 = par_table_values(P, 96, 64, 1e-18L, 4);
        printf("resonator 0.997: K = %d (T = 128), %d (T = 96); complex64 %d, %d; float64 %d; complex128 %d\n", v128.K, v96.K,
               par_table_values(P, 128, 32, 1e-18L, 4).K, par_table_values(P, 96, 32, 1e-18L, 4).K, par_table_values(P, 64, 64, 1e-30L, 8).K,
               par_table_values(P, 64, 32, 1e-30L, 8).K);
        EXPECT(!v128.failed && v128.K >= 2 && !v96.failed && v96.K >= 2);
    }

    // ---- par_upj_values: 1 / (1 - 0.5 q + 0.25 q^2), A = [0.5, -0.25; 1, 0]: dyadic entries, exact products
    {
        const double c[5] = {1.0, 0.0, 0.0, -0.5, 0.25};
        ParExpansion P;
        EXPECT(par_expand(c, 1, P));
        EXPECT(P.al[0] == 0.5 && P.be[0] == -0.25);
        const int L = 12;
        const std::vector<double> tab = par_upj_values(P, L);
        EXPECT(tab.size() == (size_t)(L + 1) * 2 + 4);   // (up to 4 biquads: row 0 once more)
        const double A[4] = {0.5, -0.25, 1.0, 0.0};
        EXPECT(tab[0] == P.al[0] && tab[1] == P.be[0]);
        for (int j = 0; j + 1 < L; ++j)
            EXPECT(tab[2 * (j + 1)] == tab[2 * j] * A[0] + tab[2 * j + 1] * A[2] && tab[2 * (j + 1) + 1] == tab[2 * j] * A[1] + tab[2 * j + 1] * A[3]);
        EXPECT(tab[2 * L] == tab[0] && tab[2 * L + 1] == tab[1]);
        double M[4] = {1.0, 0.0, 0.0, 1.0};
        for (int j = 0; j < L; ++j) {
            const double m[4] = {M[0] * A[0] + M[1] * A[2], M[0] * A[1] + M[1] * A[3], M[2] * A[0] + M[3] * A[2], M[2] * A[1] + M[3] * A[3]};
            for (int i = 0; i < 4; ++i) M[i] = m[i];
        }
        for (int i = 0; i < 4; ++i) EXPECT(tab[2 * (L + 1) + i] == M[i]);
    }

    // ---- par_v32_probe: nothing to scale the error by is the full error
    {
        ParExpansion P;
        P.nsec = 1;
        P.l1h = nan;
        EXPECT(par_v32_probe(P, 96) == 1.0);
        const double c[5] = {1.0, 0.0, 0.0, -0.5, 0.0};   // (and a benign filter is far below the limit)
        EXPECT(par_expand(c, 1, P) && par_v32_probe(P, 128) < kParV32Limit);
    }

    // ---- the stage image and the decimating stores
    EXPECT(par_stage_image_bytes(4) == 9216 && par_stage_image_bytes(8) == 17408);
    EXPECT(par_dec_rounds(4, 2, 1) && par_dec_rounds(4, 3, 1) && !par_dec_rounds(4, 4, 1) && !par_dec_rounds(8, 2, 1) && !par_dec_rounds(4, 2, 0));
    EXPECT(!par_dec_compact(4, false, 2, 6144, true, 0, 1) && par_dec_compact(4, false, 2, 6144, true, kParPlanStageM2, 1));
    EXPECT(par_dec_compact(4, false, 4, 8192, false, 0, 1) && !par_dec_compact(4, false, 3, 8192, false, 0, 1) && !par_dec_compact(4, false, 4, 8192, false, 0, 0));

    // ---- par_choose: one row per decision (n = 25200 is divisible by every factor)
    const int64_t n = 25200;
    auto is = [](const ParChoice &c, int slot, int TT, bool UPJ, int UPS, int DECM) {
        return c.status == 0 && c.slot == slot && c.TT == TT && c.UPJ == UPJ && c.UPS == UPS && c.DECM == DECM;
    };
    for (int ns : {2, 4, 5, 8}) {
        ParChoice c = choose(ns, false, false, 1, 1, 1, n);            // float32 plain
        EXPECT(is(c, 0, 0, false, 0, 0) && !c.dec_compact && c.dec_rounds == 1 && c.v32_wanted == (ns >= 7));
        EXPECT(is(choose(ns, true, false, 3, 1, 1, n), 1, 0, false, 0, 0));     // float64, three rows
        EXPECT(is(choose(ns, false, true, 1, 1, 1, n), 2, 0, false, 0, 0));     // complex64
        EXPECT(is(choose(ns, true, true, 1, 1, 1, n), 3, 0, false, 0, 0));      // complex128
        c = choose(ns, false, false, 1, 3, 1, n);                      // float32 .dn(3)
        EXPECT(is(c, 4, 96, false, 0, 1) && c.dec_compact && c.dec_rounds == 1 && !c.v32_wanted);   // (.dn never: the kept outputs' peak is not the probe's scale)
        c = choose(ns, false, false, 1, 2, 1, n);                      // float32 .dn(2): ranges of chunks up to 4 biquads, the larger image beyond
        EXPECT(ns > 4 ? is(c, 4, 96, false, 0, 3) && c.dec_compact && c.dec_rounds == 1 : is(c, 4, 96, false, 0, 2) && !c.dec_compact && c.dec_rounds == 2);
        EXPECT(!c.v32_wanted);
        c = choose(ns, false, false, 1, 5, 1, n);                      // float32 .dn(5): 5 does not divide 96
        EXPECT(is(c, 0, 0, false, 0, 1) && c.dec_compact && !c.v32_wanted);
        ParOptions o = kDefaults;
        o.iir_dn_t96 = 0;
        c = choose(ns, false, false, 1, 2, 1, n, o);                   // float32 .dn(2), iir_dn_t96 = 0
        EXPECT(is(c, 0, 0, false, 0, 2) && !c.dec_compact && c.dec_rounds == 2 && !c.v32_wanted);
        o.iir_dn_t96 = 3;
        c = choose(ns, false, false, 1, 2, 1, n, o);                   // iir_dn_t96 = 3: M = 2 keeps its ranges for every cascade
        EXPECT(is(c, 4, 96, false, 0, 2) && c.dec_rounds == 2);
        c = choose(ns, true, false, 1, 3, 1, n);                       // float64 .dn(3)
        EXPECT(is(c, 1, 0, false, 0, 1) && c.dec_compact && !c.v32_wanted);
        for (int dt = 0; dt < 4; ++dt) {
            const bool dbl = (dt & 1) != 0, il = (dt & 2) != 0;
            const int plain = (dbl ? 1 : 0) + (il ? 2 : 0), s96 = (dbl ? 6 : 4) + (il ? 1 : 0);
            for (int L : {12, 8}) {
                c = choose(ns, dbl, il, 1, 1, L, n);
                EXPECT(is(c, s96, 96, true, 0, 0) && !c.v32_wanted);
            }
            c = choose(ns, dbl, il, 1, 1, 3, n);
            EXPECT(dbl ? is(c, plain, 0, false, 0, 0) : is(c, 4 + (il ? 1 : 0), 96, false, 3, 0));
            EXPECT(is(choose(ns, dbl, il, 1, 1, 2, n), plain, 0, false, 2, 0));
            EXPECT(is(choose(ns, dbl, il, 1, 1, 4, n), plain, 0, false, dbl ? 0 : 4, 0));
            for (int L : {5, 10}) {
                c = choose(ns, dbl, il, 1, 1, L, n);
                EXPECT(is(c, plain, 0, false, 0, 0) && c.v32_wanted == (!dbl && ns >= 7 && L < 8));
            }
            EXPECT(choose(ns, dbl, il, 1, 1, 2, n).v32_wanted == (!dbl && ns >= 7));
        }
        o = kDefaults;
        o.iir_up_jump = 0;
        EXPECT(is(choose(ns, false, false, 1, 1, 12, n, o), 0, 0, false, 0, 0));
        o = kDefaults;
        o.iir_up_lean = 0;
        EXPECT(is(choose(ns, false, false, 1, 1, 2, n, o), 0, 0, false, 0, 0) && is(choose(ns, false, false, 1, 1, 3, n, o), 0, 0, false, 0, 0));
        o = kDefaults;
        o.iir_dn_compact = 0;
        c = choose(ns, false, false, 1, 3, 1, n, o);                   // no gathering store: the 128-sample image-and-pick kernel
        EXPECT(is(c, 0, 0, false, 0, 1) && !c.dec_compact && c.dec_rounds == 1);
        EXPECT(choose(ns, false, true, 1, 3, 1, n, o).status == 1);    // (interleaved signals have no other decimating store)
        o = kDefaults;
        o.iir_par_v32 = 0;
        EXPECT(!choose(ns, false, false, 1, 1, 1, n, o).v32_wanted);
    }
    // not served
    EXPECT(choose(4, false, true, 3, 1, 1, n).status == 1);     // interleaved, more than one row
    EXPECT(choose(4, false, false, 1, 3, 2, n).status == 1);    // up with dec
    EXPECT(choose(4, false, false, 1, 1, 11, n).status == 1);   // n % up != 0
    EXPECT(choose(4, false, false, 3, 1, 2, n).status == 1);    // up, more than one row
    EXPECT(choose(9, false, false, 1, 1, 1, n).status == 1 && choose(0, false, false, 1, 1, 1, n).status == 1);
    {   // a 96-sample choice whose slot reports K = 0 falls back to the 128-sample tables; the K query is asked in the order the tables are made
        Asked a;
        ParChoice c = choose(8, false, false, 1, 3, 1, n, kDefaults, 0, &a);
        EXPECT(is(c, 0, 0, false, 0, 2) && !c.dec_compact && c.dec_rounds == 2 && (a.slots == std::vector<int>{4, 0}));   // (M = 3 on 128-sample chunks: ranges of chunks)
        a.slots.clear();
        c = choose(8, false, true, 1, 1, 12, n, kDefaults, 0, &a);
        EXPECT(is(c, 2, 0, false, 0, 0) && !c.v32_wanted && (a.slots == std::vector<int>{5, 2}));
        a.slots.clear();
        c = choose(8, false, false, 1, 1, 1, n, kDefaults, 1, &a);
        EXPECT(a.slots == std::vector<int>{0});                   // a plain call never asks for (and so never builds) a 96-sample table
        c = par_choose(8, false, false, 1, 1, 1, n, kDefaults, [](int) { return 0; });
        EXPECT(c.status == 1);
        c = par_choose(8, false, false, 1, 3, 1, n, kDefaults, [](int) { return -3; });
        EXPECT(c.status == -3);                                   // an error of the query is passed on
    }
    // the table slots
    EXPECT(par_slot_T(0) == 128 && par_slot_T(1) == 64 && par_slot_T(2) == 128 && par_slot_T(3) == 64 && par_slot_T(4) == 96 && par_slot_T(7) == 96);
    EXPECT(par_slot_chunks(0) == 64 && par_slot_chunks(2) == 32 && par_slot_chunks(3) == 32 && par_slot_chunks(4) == 64 && par_slot_chunks(5) == 32 &&
           par_slot_chunks(6) == 64 && par_slot_chunks(7) == 32);
    EXPECT(!par_slot_dbl(0) && par_slot_dbl(1) && par_slot_dbl(3) && !par_slot_dbl(4) && !par_slot_dbl(5) && par_slot_dbl(6) && par_slot_dbl(7));

    if (g_fail) {
        printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("OK\n");
    return 0;
}
