// fir_route.hpp -- which engine a FIR call runs: the applicability rule of every FIR engine, the geometry of the matrix-pipe kernels, the
// measured cost models, tap segments and heads, and fir_route -- ONE decision per call, which fir_api.hip (fir_run) executes.  Standard
// headers only: it compiles without a device toolchain, and tests/host/fir_route_emul.cpp runs it on the host against the recorded table
// tests/fir_routes/mi355x.txt.  Every engine's *_launch checks its own predicate from here, so a launch and the router cannot disagree.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>
#include "ols_tables.hpp"

namespace skdsp {

// the codes of include/skdsp.h this header reads (fir_api.hip ties each to its own with a static_assert)
enum { kFirF32 = 0, kFirC64 = 1, kFirF64 = 2, kFirC128 = 3 };
enum { kFirAuto = 0, kFirDirect = 1, kFirOls = 2 };

using ols::tile_overlap;
using ols::up_passes;
using ols::up_taps_per_phase;

// what the decision reads of a handle
struct FirShape {
    int dtype, ntaps;
    bool taps_complex;
    int algo;   // skdsp_fir_set_algo
};
template <class H> inline FirShape fir_shape_of(const H *h) { return FirShape{h->dtype, h->ntaps, h->taps_complex, h->algo}; }
inline bool fir_dbl(const FirShape &s) { return s.dtype == kFirF64 || s.dtype == kFirC128; }
inline bool fir_cplx(const FirShape &s) { return s.dtype == kFirC64 || s.dtype == kFirC128; }
inline int fir_esz(const FirShape &s) { return s.dtype == kFirF32 ? 4 : (s.dtype == kFirC128 ? 16 : 8); }

// the options FIR dispatch reads (struct Options in skdsp_internal.hpp; fir_api.hip fills it)
struct FirRouteOptions {
    int fir_algo = kFirAuto, dn_no_ols = 0, fir_mm = 1, fir_bx = 1, fir_up_ols_min = 64, fir_up_rows_min = -1, fir_up_pair = 1, fir_up4k = 1, fir_up2k = 1,
        fir_up_rep = 1, fir_dn_fold = 1, fir_dn4k = 1, fir_updn_fused = 1;
};

// one call of an entry point
struct FirCall {
    int64_t n, n_hist;
    int L, M;
    bool plain;          // .filter (L = M = 1; the rate changers with L = M = 1 take no head and never the frequency domain)
    unsigned y_low;      // the low address bits of y (the pairs forms test them)
    bool scratch_free;   // workspace slot 2 is free (false inside a tap-segment call, which holds it)
    int num_cus;
};

// ---- applicability of the engines -------------------------------------------------------------------------------------------
// overlap-save (fir_ols.hip): complex64 with any taps; float32 with real taps (two real tiles per complex tile)
inline bool fir_ols_supported(const FirShape &h)
{
    // complex64 signal; overlap must leave at least half the tile as useful output
    if (h.ntaps < 2 || h.ntaps - 1 > 4096) return false;
    return h.dtype == kFirC64 || (h.dtype == kFirF32 && !h.taps_complex);
}
inline bool fir_ols_up_supported(const FirShape &h, int L)
{
    if (L < 2 || L > 256) return false;   // (the every-M-th store: L <= 64, checked at launch)
    const int T = up_taps_per_phase(h.ntaps, L);
    if (T < 2 || T - 1 > 4096) return false;
    return h.dtype == kFirC64 || (h.dtype == kFirF32 && !h.taps_complex);
}
// float32 signals, no decimation: the phases run in pairs through the complex tile (load_tile_xr).  Even L: an 8-byte aligned destination
// (L / 2 rows of pairs in the rows form).  Odd L (7 .. 13, strided form only): (L - 1) / 2 pairs as 8-byte elements at 4-byte aligned
// addresses, then the last phase on its own (two real tiles per pass) -- L passes per two tiles either way.  Measured against one phase
// per pass (2^26 outputs, 256 taps per phase): L = 7 0.237 -> 0.216 ms, 9 0.248 (rows) -> 0.209, 11 0.255 -> 0.229, 13 0.254 -> 0.245;
// L = 3, 5 lose (0.168 -> 0.186, 0.200 -> 0.208: the misaligned 8-byte stores and the second launch), 15 loses to the rows form.
inline bool fir_ols_up_pairs(const FirShape &h, int L, int dec, unsigned y_low, int fir_up_pair)
{
    if (!fir_up_pair || h.dtype != kFirF32 || h.taps_complex || dec > 1) return false;
    if (L % 2 == 0) return (y_low & 7) == 0;
    return L >= 7 && L <= 13 && (y_low & 3) == 0;
}
// multirate_FIR.up, even L, at most 4097 taps in all: tiles of the OUTPUT (ols_rep_kernel)
inline bool fir_ols_rep_supported(const FirShape &h, int L, int fir_up_rep)
{
    if (L < 2 || L % 2 || L > 4096 || !fir_up_rep) return false;
    return fir_ols_supported(h);
}
// the tile interpolators: complex64 (any taps) or float32 with real taps; per phase at most 2049 (fir_up4k.hip) / 1025 (fir_up2k.hip) taps (half a tile of overlap)
inline bool fir_up_tile_supported(const FirShape &h, int L, int max_overlap)
{
    // (a plan holds one 32 / 16 KiB table per pass, built on first use under the handle's lock: 256 passes are 8 / 4 MiB and a few ms of host transforms;
    // beyond that the walk over (tile, phase) pairs and the polyphase kernels serve the call)
    if (L < 2 || L > 256) return false;
    if (up_taps_per_phase(h.ntaps, L) - 1 > max_overlap) return false;
    return h.dtype == kFirC64 || (h.dtype == kFirF32 && !h.taps_complex);
}
inline bool fir_up4k_supported(const FirShape &h, int L) { return fir_up_tile_supported(h, L, 2048); }
inline bool fir_up2k_supported(const FirShape &h, int L) { return fir_up_tile_supported(h, L, 1024); }
// the frequency-domain decimator (fir_dn4k.hip): per phase at most 2049 taps
inline bool fir_dn4k_supported(const FirShape &h, int M)
{
    if (M < 2 || M > 4) return false;   // (one load group: all phases of a sample in one thread)
    if (ols::dn_taps_per_phase(h.ntaps, M) - 1 > 2048) return false;
    return h.dtype == kFirC64 || (h.dtype == kFirF32 && !h.taps_complex);
}
// overlap-save in float64 (fir_ols64.hip): complex128, and float64 with real taps; 2..2049 taps (per phase)
inline bool fir_ols64_supported(const FirShape &h)
{
    if (h.ntaps < 2 || h.ntaps - 1 > 2048) return false;
    return h.dtype == kFirC128 || (h.dtype == kFirF64 && !h.taps_complex);
}
inline bool fir_ols64_up_supported(const FirShape &h, int L)
{
    if (L < 2 || L > 256) return false;   // (the every-M-th store: L <= 64, checked at launch)
    const int T = up_taps_per_phase(h.ntaps, L);
    if (T < 2 || T - 1 > 2048) return false;
    return h.dtype == kFirC128 || (h.dtype == kFirF64 && !h.taps_complex);
}
// float64 signals, real taps, even L, no decimation, a 16-byte aligned destination: the phases run in pairs through the complex tile
inline bool fir_ols64_up_pairs(const FirShape &h, int L, int dec, unsigned y_low, int fir_up_pair)
{
    return fir_up_pair && h.dtype == kFirF64 && !h.taps_complex && L % 2 == 0 && dec <= 1 && (y_low & 15) == 0;
}

// Toeplitz product on the FP32 / FP64 matrix pipe (fir_mm.hip): real taps, not complex128
constexpr int kMmPlanStepsF = 96, kMmPlanStepsD = 48;   // the most 4-lag steps fir_mm.hip instantiates (it ties them with a static_assert)
inline bool fir_mm_supported(const FirShape &h, int L, int M, int64_t n_out)
{
    if (h.taps_complex || h.dtype == kFirC128) return false;  // complex128: the sliding-window kernel measured faster
    const int kmax = fir_dbl(h) ? kMmPlanStepsD : kMmPlanStepsF;  // A operands in registers: 1 (float) or 2 (double) VGPRs per step
    const int g = std::gcd(L, M), Lp = L / g, q = M / g;
    if (Lp > 16) return false;
    const int T = (h.ntaps + L - 1) / L, DS = 16 / Lp;
    const int64_t imax = ((int64_t)(Lp - 1) * M) / L;
    const int64_t K = T + imax + (int64_t)q * (DS - 1);
    if (K > 4 * kmax - 12) return false;                  // A operands must fit the register file
    const int64_t win = (int64_t)q * DS * 63 + K + 32;    // smallest workgroup tile (NS = 64)
    if (win * 9 / 8 * (int64_t)fir_esz(h) > 63 * 1024) return false;
    return n_out >= 16 * 64;
}

// ---- the fp16-piece matrix-pipe kernels (fir_bx.hip): geometry ---------------------------------------------------------------
// the kernel's constants this code depends on (fir_bx.hip ties each to its own with a static_assert)
constexpr int kBxPlanUnitsC = 512, kBxPlanUnitsR = 1024;     // kBxUnitsC / kBxUnitsR: 8-sample units of one window
constexpr int kBxPlanUnitsCK = 896, kBxPlanUnitsRK = 2048;   // kBxUnitsCK / kBxUnitsRK: ... of the lag-split kernels (KSP = 4)
constexpr int kBxPlanPx = 2, kBxPlanPh = 2;                  // kBxPx / kBxPh: fp16 pieces of a sample / of a tap
constexpr int bx_units(bool cplx, bool ksp) { return ksp ? (cplx ? kBxPlanUnitsCK : kBxPlanUnitsRK) : (cplx ? kBxPlanUnitsC : kBxPlanUnitsR); }

// does a wave's share fit its 256 VGPRs (2 waves per SIMD)?  A operands (4 per tap piece, 32-lag block and row tile) + accumulators + B
// fragments + 32 prefetch registers + ~60 others; kb, rt: blocks / row tiles PER WAVE.  Used by the geometry below and by the dispatch, so
// that only kernels the geometry can pick are instantiated.
constexpr bool bx_fits(bool cplx, int kb, int rt)
{
    return kb * rt <= 16 && 4 * kBxPlanPh * kb * rt + 8 * (cplx ? 2 : 1) * rt + 4 * kBxPlanPx * (cplx ? 2 : 1) + 32 + 60 <= 252;
}

// RT / KB: row tiles / 32-lag blocks of the table; RSP / KSP: waves they are dealt to
struct BxGeometry { int L, M, Lp, q, DS, RS, RT, U0, KB, RSP, KSP; };

// geometry of one (L, M): false if the kernel family does not cover it (G: BxGeometry, or the table that derives from it -- BxTab of fir_bx.hip)
template <class G> inline bool bx_geometry(const FirShape &h, int L, int M, G *t)
{
    const int g = std::gcd(L, M), Lp = L / g, q = M / g;
    const int P = h.ntaps, T = (P + L - 1) / L;
    const int ds0 = 8 / std::gcd(q, 8);  // q DS must be a multiple of 8
    int best_k = 0;
    double best_util = 0.0;
    for (int k = 1; k <= 16; ++k) {
        const int RS = Lp * ds0 * k, RT = (RS + 15) / 16;
        if (RT > 8) break;
        const double util = (double)RS / (16.0 * RT);
        if (util > best_util + 1e-9) { best_util = util; best_k = k; }
    }
    if (best_k == 0 || best_util < 0.74) return false;
    const int comp = fir_cplx(h) ? 2 : 1;
    const int al = comp == 2 ? 2 : 4;
    const int cap = 8 * (comp == 2 ? kBxPlanUnitsC : kBxPlanUnitsR);
    int DS, RS, RT, U0, KB;
    for (;; best_k /= 2) {
        DS = ds0 * best_k; RS = Lp * DS; RT = (RS + 15) / 16;
        int imax = 0;
        for (int c = 0; c < Lp; ++c) imax = std::max(imax, (int)(((int64_t)c * M) / L));
        U0 = imax + q * (DS - 1);
        // window element 0 is input q_ds S0 + U0 + 1 - 32 KB: a 16-byte boundary of x for U0 + 1 = 0 mod 4 (2 for complex)
        U0 += (al - (U0 + 1) % al) % al;
        KB = (T + U0 + 31) / 32;
        // A decimator with a large M (one class, one row tile): 16 slots per column are 16 M inputs, and 16 columns of them may not fit the
        // window (M = 24: 16 x 384 samples).  Fewer slots per column then -- half-empty row tiles cost matrix-pipe time these shapes do
        // not lack (M = 24, 512 taps, complex64: 1.43 ms per 2^26 inputs on the kernels behind this one).
        if (Lp > 1 || best_k % 2 || RS < 8 || 8 * bx_units(comp == 2, true) >= q * DS * 15 + 32 * ((KB + 3) / 4 * 4)) break;
    }
    // What does not fit one wave (bx_fits) is tried with the row tiles dealt to wave pairs (RSP = 2: see the kernel); four or more row tiles
    // always are (the same speed where both fit -- L = 8, 48 taps per phase: 0.1245 / 0.1259 ms -- and the one-wave forms of 4 x 2, 6 x 1 spilled)
    int RSP = 0;
    const bool pairs_first = RT >= 4 && RT % 2 == 0;
    for (int i = 0; i < 2 && !RSP; ++i) {
        const int rsp = (i == 0) == pairs_first ? 2 : 1;
        if (RT % rsp || (rsp > 1 && RT < 4)) continue;
        if (bx_fits(comp == 2, KB, RT / rsp)) RSP = rsp;
    }
    // One row tile and a window that holds fewer column tiles than the workgroup has waves (a decimator with a large M), or more blocks
    // than one wave's registers take: the waves split the lags (KSP = 4: see the kernel); the table is padded to 4 equal shares.
    int KSP = 1, KBT = KB;
    if (RT == 1) {
        const int ns_max = cap > 32 * KB ? (cap - 32 * KB) / (q * DS) + 1 : 0;
        if (!RSP || ns_max < 64) {
            const int kbw = (KB + 3) / 4;
            if (kbw <= 12 && 8 * bx_units(comp == 2, true) >= 32 * 4 * kbw + q * DS * 15) { KSP = 4; KBT = 4 * kbw; RSP = 1; }
        }
    }
    if (!RSP) return false;
    t->RSP = RSP;
    t->KSP = KSP;
    t->L = L; t->M = M; t->Lp = Lp; t->q = q; t->DS = DS; t->RS = RS; t->RT = RT; t->U0 = U0; t->KB = KBT;
    return true;
}

template <class G> inline int bx_columns(const G *t, int comp, int64_t n_out, int num_cus)
{
    // columns per workgroup: what a window of kBxUnitsC / kBxUnitsR 8-sample units holds (32 KiB of fp16 planes: 3
    // workgroups per CU by LDS, 2 by registers), multiples of 64 (16 for wide strides), at most 512
    auto win_of = [&](int NS) { return ((t->q * t->DS * (NS - 1) + 32 * t->KB) + 7) / 8 * 8; };
    const int cap = 8 * bx_units(comp == 2, t->KSP > 1);
    int NS = 512;
    while (NS > 64 && win_of(NS) > cap) NS -= 64;
    while (NS > 16 && win_of(NS) > cap) NS -= 16;
    if (win_of(NS) > cap) return 0;
    const int64_t ncols = (n_out + t->RS - 1) / t->RS;
    while (NS > 64 && (ncols + NS - 1) / NS < 2 * num_cus) NS -= 64;  // small problems: more windows
    return NS;
}

inline bool fir_bx_supported(const FirShape &h, int L, int M, int64_t n_out, int num_cus)
{
    if (h.taps_complex || fir_dbl(h)) return false;
    BxGeometry t;
    if (!bx_geometry(h, L, M, &t)) return false;
    if (bx_columns(&t, fir_cplx(h) ? 2 : 1, n_out, num_cus) == 0) return false;
    return n_out >= (int64_t)t.RS * 64;
}

// 32-lag blocks the kernel would run for (L, M); 0: not covered (the cost models)
inline int fir_bx_blocks(const FirShape &h, int L, int M, const FirRouteOptions &o, int *row_tiles = nullptr)
{
    if (h.taps_complex || fir_dbl(h)) return 0;
    if (!o.fir_bx || !o.fir_mm) return 0;
    BxGeometry t;
    if (!bx_geometry(h, L, M, &t)) return 0;
    if (row_tiles) *row_tiles = t.RT;
    return t.KB;
}

// The polyphase launcher (fir_direct.hip) has a kernel for (L, M) unless the register sliding window with R = 2 outputs per thread exceeds its
// 80 KiB of LDS (a larger R only needs more) AND the generic kernel's 64 KiB window has no room for one output slot per class.
inline bool fir_direct_holds(const FirShape &h, int L, int M)
{
    const int g = std::gcd(L, M), q = M / g;
    const int T = (h.ntaps + L - 1) / L;
    const int64_t esz = fir_esz(h);
    const int Tq = (T + q - 1) / q, nB = (Tq + 1 + 2 - 1) / 2;
    if ((int64_t)(nB + 256) * (2 * (int64_t)q + 1) * esz <= 80 * 1024) return true;
    return (65536 / esz - T - q) / q >= 1;
}

// ---- what one call runs ------------------------------------------------------------------------------------------------------
enum FirEngine {
    kRouteNone = 0,     // no output: nothing is launched
    kRouteRefused,      // SKDSP_ERR_UNSUPPORTED (the launcher that refuses says why)
    kRouteBx, kRouteMm, kRouteDirect,   // the tiers of the polyphase launcher: fp16-piece matrix pipe, FP32 / FP64 matrix pipe, sliding window or generic
    kRouteOls, kRouteOls64,             // overlap-save; dec > 1: the decimating store (float32 signals, even M: the folded inverse, option fir_dn_fold)
    kRouteDn4k, kRouteUp4k, kRouteUp2k, kRouteOlsRep,
    kRouteWalk, kRouteWalk64,           // the overlap-save walk over (tile, phase) pairs
    kRouteParts,                        // tap segments of `seg` taps, each routed on its own shape
};
enum FirCopy {
    kCopyNone = 0,
    kCopyWeave,      // the walk leaves rows in workspace slot `slot`; interleave_launch weaves them
    kCopyEveryMth,   // the walk writes all n L outputs to workspace slot `slot`; every M-th is copied
    kCopyFullRate,   // the full-rate filter (engine, head: as .filter routes it) into workspace slot `slot`, and a strided copy
};
struct FirRoute {
    int engine = kRouteNone;
    int L = 1, M = 1;
    bool paired = false, rows = false;   // the walk: phases in pairs, phases as rows
    int dec = 1;                         // the decimating store of overlap-save and of the walk
    int copy = kCopyNone, slot = 2;
    bool direct_refused = false;         // the polyphase launcher has no kernel for the stride, and the route is what serves the call instead (the path notes the launcher first)
    int seg = 0;                         // > 0: the call runs as tap segments of this many taps
    int head = 0;                        // > 0: the call runs on the filter's first `head` taps
};

// FIR .filter algorithm choice.  OLS needs complex64; it wins once direct form stops
// being HBM-bound (2*P FMA per c64 sample on the VALU vs ~120 flop in the FFT domain).
inline int pick_fir_algo(const FirShape &h, int64_t n, const FirRouteOptions &o)
{
    int algo = o.fir_algo != kFirAuto ? o.fir_algo : h.algo;
    const bool ols64 = fir_ols64_supported(h);
    if (algo == kFirOls && !fir_ols_supported(h) && !ols64) algo = kFirDirect;
    if (algo != kFirAuto) return algo;
    // float64 signals: the direct form costs 2 (4 for complex taps) FP64 FMA per tap and real sample; the float64
    // overlap-save tile is flat in the tap count (measured crossovers at 2^26 samples: see DESIGN.md 4.2, LABNOTES.md)
    if (ols64) return h.ntaps >= (h.dtype == kFirC128 ? 24 : 128) && n >= 8192 ? kFirOls : kFirDirect;
    // measured crossover at 2^26 samples (tools/time_fir_filter.py, profiles/r04/fir_filter.txt): the matrix-pipe kernel (real taps, fp16 pieces)
    // stays ahead of overlap-save up to 6 lag blocks for complex64 (0.215 vs 0.229 ms at 145 taps; 0.221 vs 0.227 at 160; 0.241 vs 0.227 at 192)
    // and for float32 (0.109 vs 0.125 ms at 145 taps; 0.125 vs 0.126 at 192; 0.133 vs 0.122 at 224)
    const int ols_from = h.taps_complex ? 48 : (h.dtype == kFirC64 ? 177 : 193);
    if (fir_ols_supported(h) && h.ntaps >= ols_from && n >= 4096) return kFirOls;
    return kFirDirect;
}

// ---- tap segments and heads --------------------------------------------------------------------------------------------------
// per launch: 4097 taps (float32 overlap-save / direct) or 2049 (float64); an interpolator holds ceil(Ntaps / L) per phase
inline int fir_part_len(const FirShape &h) { return fir_dbl(h) ? 2048 : 4096; }
inline bool fir_needs_parts(const FirShape &h, int L = 1) { return up_taps_per_phase(h.ntaps, L) > (fir_dbl(h) ? 2049 : 4097); }
// taps per segment: a multiple of lcm(L, M), at most fir_part_len taps per phase
inline int fir_parts_seg(const FirShape &h, int L, int M)
{
    const int lcm = L / std::gcd(L, M) * M;
    return std::max(fir_part_len(h) * L / lcm, 1) * lcm;
}
inline int fir_parts_count(const FirShape &h, int seg) { return (h.ntaps + seg - 1) / seg; }
// lcm(L, M) beyond what a launch takes per phase: no segment length serves the call (refused; it used to cut its one segment again, without end)
inline bool fir_parts_seg_ok(const FirShape &h, int seg, int L) { return !fir_needs_parts(FirShape{h.dtype, std::min(seg, h.ntaps), h.taps_complex, h.algo}, L); }
// A segment may start inside the history only by whole output periods (q = M / gcd inputs).  A history that covers a segment's
// delay is used in full; a shorter one is used up to a multiple of q -- if it is not one itself, the samples
// x[-n_hist .. -d-1] would be dropped from the outputs just below that segment's first one, so such a call is refused
// (the host pipeline and the sharded path always hand over a history that is complete or a multiple of q).
inline bool fir_parts_history_ok(const FirShape &h, int seg, int L, int M, int64_t n_hist)
{
    const int q = M / std::gcd(L, M);
    const int64_t last_delay = (int64_t)(fir_parts_count(h, seg) - 1) * seg / L;
    return q == 1 || n_hist >= last_delay || n_hist % q == 0;
}
// segment si of a call: the taps it holds and the call it is (x moved d samples into the history, `off` the first output it adds to, cnt how many)
struct FirSegment { int t0, taps; int64_t d, n, n_hist, off, cnt; };
inline bool fir_parts_segment(const FirShape &h, int seg, int si, int64_t n, int64_t n_hist, int L, int M, FirSegment *out)
{
    const int q = M / std::gcd(L, M);
    const int64_t n_out = (n * L) / M;
    const int64_t delay_in = (int64_t)si * seg / L, delay_out = (int64_t)si * seg / M;
    out->t0 = si * seg;
    out->taps = std::min(seg, h.ntaps - out->t0);
    out->d = (std::min(n_hist, delay_in) / q) * q;       // how far this segment starts inside the history
    out->n = n - delay_in + out->d;
    out->n_hist = n_hist - out->d;
    out->off = delay_out - out->d * L / M;                // first output this segment contributes to
    out->cnt = std::min((out->n * L) / M, n_out - out->off);
    return out->taps > 0 && out->n > 0 && out->cnt > 0;
}
// A call from rest over n < Ntaps samples only ever reaches the first n taps: it runs on the filter cut to the next power of two >= n (0: on the filter itself)
inline int fir_head_taps(int ntaps, int64_t n)
{
    if (n >= ntaps || n < 1) return 0;
    int keep = 1;
    while (keep < n) keep <<= 1;
    return keep >= ntaps ? 0 : keep;
}

// ---- multirate_FIR.up: the cost model ----------------------------------------------------------------------------------------
// multirate_FIR.up through the overlap-save walk: from which L on the phases leave as rows of scratch and a second kernel weaves them
// (measured crossovers of profiles/r03/fir_up.txt -- the walk serves float64 and > 1025 taps per phase today; 16-byte samples never: their strided stores are full-width requests already)
inline bool fir_up_rows(const FirShape &h, int L, const FirRouteOptions &opt, bool paired = false)
{
    const int o = opt.fir_up_rows_min;
    if (o == 0) return false;
    if (o > 0) return L >= o;
    if (paired) return !fir_dbl(h) && L % 2 == 0 && L / 2 >= 7;   // (8-byte pairs: the complex64 crossover, in phases; 16-byte pairs never;
                                                                  //  odd L in pairs: the strided form only)
    switch (h.dtype) {
    case kFirF32: return L >= 9;
    case kFirC64: return L >= 7;
    case kFirF64: return L >= 6;
    default: return false;
    }
}

// The one-workgroup-per-input-tile interpolators (fir_up4k.hip: up to four passes per thread; fir_up2k.hip: all passes of a row per
// thread): which one a call takes (0: none applies), and what it costs in ms per 2^26 outputs on this board (round-4 timings,
// tools/time_up4k.py; the measured shapes had 3 - 6 % of their tile in the overlap, so the figure is scaled to the call's overlap).
inline int fir_up_tile_kind(const FirShape &h, int L, const FirRouteOptions &opt)
{
    if (fir_dbl(h) || !opt.fir_up4k) return 0;
    const int passes = up_passes(L, h.dtype == kFirF32);   // (float32: two phases per complex pass)
    // float32, L = 2: one pass -- the walk's pair form IS the plain filter's 8192-point tile with an 8-byte store, and stays ahead of the
    // 4096-point tile (512 / 1024 taps per phase: 0.117 / 0.125 ms against 0.126 / 0.140)
    if (passes == 1 && opt.fir_up4k < 2) return 0;
    if (opt.fir_up2k && fir_up2k_supported(h, L) && (opt.fir_up2k >= 2 || passes > 4)) return 2;
    return fir_up4k_supported(h, L) ? 4 : 0;
}
inline double fir_up_tile_ms(const FirShape &h, int L, int kind, int *V_out)
{
    const int T = up_taps_per_phase(h.ntaps, L);
    const int passes = up_passes(L, h.dtype == kFirF32);
    const bool cplx = h.dtype == kFirC64;
    double ms;
    int N, ov;
    if (kind == 4) {   // 4096-point tile, groups of four passes: one group is one burst per row, more are pieces written far apart
        N = 4096; tile_overlap(T, 256, N, &ov, V_out);
        // (one group: the forward transform is shared by `passes` inverse ones -- 0.2025 / 0.199 / 0.187 ms at 2 / 3 / 4 complex64 passes,
        // 0.1225 / 0.0946 / 0.105 / 0.096 at 1 .. 4 float32 passes, profiles/r04/fir_up.txt)
        static const double c4[5] = {0.0, 0.26, 0.2025, 0.199, 0.187}, f4[5] = {0.0, 0.1225, 0.0946, 0.105, 0.096};
        ms = cplx ? (passes <= 4 ? c4[passes] : 0.30 + 0.012 * std::min(passes, 12)) : (passes <= 4 ? f4[passes] : 0.10 + 0.005 * std::min(passes, 12));
        ms *= (4096.0 - 256.0) / 4096.0;
    } else {           // 2048-point tile, up to twelve passes per thread
        N = 2048; tile_overlap(T, 64, N, &ov, V_out);
        if (passes <= 12) ms = cplx ? 0.19 + 0.0025 * passes : 0.085 + 0.0035 * passes;
        else ms = cplx ? 0.36 : 0.16;
        if (passes % 2) ms *= 1.07;   // (an odd row: every lane stores its own pieces)
        ms *= (2048.0 - 64.0) / 2048.0;
    }
    return ms * (double)N / (double)(N - ov);
}

// multirate_FIR.up, even L, on tiles of the OUTPUT (fir_ols.hip: ols_rep_kernel): ms per 2^26 outputs (round-5 timings, profiles/r05/fir_up.txt: the plain
// filter's tile with a quarter of its forward transform and 1 / L of its loads; the overlap is that of the WHOLE filter at the high rate)
inline double fir_up_rep_ms(const FirShape &h, int L)
{
    int ov, V;
    tile_overlap(h.ntaps, 512, 8192, &ov, &V);
    const bool cplx = h.dtype == kFirC64;
    const bool pow2 = (L & (L - 1)) == 0 && L <= 16;   // (else the decimated grid is itself zero-stuffed: the guarded loader, 4-byte samples feel it)
    const double base = cplx ? (L == 2 ? 0.161 : 0.152) : (L == 2 ? 0.087 : (L == 4 ? 0.083 : 0.0885)) * (pow2 ? 1.0 : 1.18);
    return base * 8192.0 / (8192.0 - ov);
}

// multirate_FIR.up: polyphase kernels or the frequency domain?  Both are timed models of this board at 2^26 outputs (tools/time_fir_up.py; ms),
// scaled to the call: the polyphase kernels cost per tap of a phase -- little where the matrix-pipe kernel covers the shape, 3-4x that where it
// does not -- the walk costs per (tile, phase) pair whatever the phase length, plus what its stride-L stores cost, and runs in rounds of one pair
// per resident workgroup.
// best: which frequency-domain engine the model found cheapest (1 the walk over (tile, phase) pairs, 2 an input-tile interpolator, 3 the output-tile one)
struct FirUpModel { bool prefers_ols = false; int best = 1; };
inline int &fir_up_model_runs() { static int runs = 0; return runs; }   // evaluations so far (tests: at most one per routed call)
inline FirUpModel fir_up_model(const FirShape &h, int L, int64_t n, int M, int num_cus, const FirRouteOptions &opt)
{
    ++fir_up_model_runs();
    FirUpModel out;
    const int T = up_taps_per_phase(h.ntaps, L);
    const int floor_t = opt.fir_up_ols_min;   // < 0: wherever supported from -floor_t taps per phase on, no cost model (tests, A/B timing)
    const bool dbl = fir_dbl(h);
    int floor_eff = std::abs(floor_t);   // (many phases: the polyphase kernels lose their reuse early -- let the cost model see shorter phases too)
    if (floor_t > 0 && L > 64) floor_eff = std::max(8, floor_t / 8);
    else if (floor_t > 0 && L > 16) floor_eff = std::max(8, floor_t / 4);
    const int kind = M == 1 ? fir_up_tile_kind(h, L, opt) : 0;
    if (M == 1 && floor_t > 0 && kind) floor_eff = std::min(floor_eff, 24);   // (the tile interpolators cross over with the polyphase kernels at short phases already)
    if (floor_t == 0 || T < floor_eff || n < 8192 || !(dbl ? fir_ols64_up_supported(h, L) : fir_ols_up_supported(h, L))) return out;
    if (M > 1 && L > 64) return out;   // (the every-M-th store's exact-division range; the scratch + copy form is not worth it there)
    out.prefers_ols = true;
    if (floor_t < 0) return out;
    out.prefers_ols = false;
    if ((opt.fir_algo != kFirAuto ? opt.fir_algo : h.algo) == kFirDirect) return out;
    out.prefers_ols = true;
    if (fir_needs_parts(h, L)) return out;   // (longer than one polyphase launch takes)
    // all figures: ms per 2^26 up-rate samples on this board (the walk and the float64 kernels: profiles/r03/fir_up.txt, fir_updn.txt; the matrix-pipe and tile kernels: profiles/r04)
    const double Lf = (double)L;
    const bool cplx = fir_cplx(h);
    double ols, base, poly, copy;   // base: the walk without what its stride-L stores cost
    int V;
    if (dbl) {   // FP64 direct taps against the float64 walk (4096-point tiles)
        base = cplx ? 0.42 : 0.26;
        ols = cplx ? 0.60 + 0.008 * std::min(Lf, 24.0) : 0.29 + 0.02 * std::min(Lf, 12.0);
        poly = cplx ? 0.5 + 0.0055 * T : (T <= 128 ? 0.17 + 0.0018 * T : 0.1 + 0.0028 * T);
        if (cplx && L > 16) poly = std::max(poly, 1.0);   // (measured 1.02 ... 1.12 from L = 24 on, whatever the phase length)
        if (T > 128) poly *= std::max(1.0, Lf / 4.0);   // (many long phases: the tap tables fall out of the cache)
        else if (L > 16 && !cplx) poly *= 1.0 + Lf / 12.0;
        copy = cplx ? 0.20 : 0.10;
        V = 4096 - ((T - 1 + 255) / 256) * 256;
    } else {
        int bx_rt = 0;
        const int bx_kb = fir_bx_blocks(h, L, M, opt, &bx_rt);   // (the matrix-pipe polyphase kernel covers the shape: its time goes with its 32-lag blocks)
        const bool bx = bx_kb > 0;
        base = cplx ? 0.23 : 0.125;
        ols = cplx ? 0.27 + 0.022 * std::min(Lf, 20.0) : 0.13 + 0.018 * std::min(Lf, 28.0);
        // profiles/r04/fir_up.txt (fp16 pieces): complex64 0.106 - 0.122 up to 3 blocks, then + 0.0145 per block (5: 0.13, 7: 0.165; one row tile, L = 2:
        // 0.122 / 0.127 / 0.143 / 0.159 / 0.194 / 0.223 for 2 / 3 / 4 / 5 / 7 / 9); float32 0.080 - 0.096 up to 5 blocks, 0.099 at 7 (L = 2: 0.075 ... 0.133)
        if (bx && cplx) poly = bx_rt == 1 ? 0.093 + 0.0145 * bx_kb : std::max(L >= 8 ? 0.118 : 0.106, 0.062 + 0.0145 * bx_kb);
        else if (bx) poly = bx_rt == 1 ? 0.058 + 0.0084 * bx_kb : std::max(0.081 * (L > 8 ? 1.15 : (L == 8 ? 1.06 : 1.0)), 0.04 + 0.0084 * bx_kb);
        else poly = cplx ? 0.02 + 0.0037 * T : 0.03 + 0.0018 * T;
        if (!bx && L > 8 && L <= 16) poly *= 1.0 + 0.05 * (Lf - 8.0);   // (48 taps per phase: 0.116 modelled, 0.1395 measured at L = 12)
        if (!bx && T > 256) poly *= std::max(1.0, Lf / 4.0);
        else if (L > 16 && !bx) poly *= 1.0 + Lf / 12.0;   // (one tap table per phase: the polyphase kernels lose their reuse)
        copy = cplx ? 0.10 : 0.06;
        V = 8192 - ((T - 1 + 511) / 512) * 512;
    }
    if (M == 1 && fir_up_rows(h, L, opt)) ols = std::min(ols, dbl ? 0.45 : (cplx ? 0.45 : 0.245));   // (rows + weave: whatever L is)
    if (M == 1 && !dbl && fir_ols_up_pairs(h, L, 1, 0, opt.fir_up_pair))   // float32, even L: L / 2 complex passes per tile of real input, 8-byte outputs
        ols = std::min(0.11 + 0.007 * Lf, 0.235);
    if (M == 1 && dbl && fir_ols64_up_pairs(h, L, 1, 0, opt.fir_up_pair))   // float64 likewise, 16-byte outputs
        ols = 0.25 + 0.005 * std::min(Lf, 16.0);
    if (M > 1) {   // L / M: the polyphase kernels compute the kept outputs only; the walk computes all and stores (or copies) every M-th
        poly /= (double)M;
        if (M <= 4096 && opt.fir_updn_fused) ols = base + (ols - base) / (double)M;
        else ols += copy;
    }
    // the walk runs in rounds of one (tile, phase) pair per resident workgroup; the polyphase kernels scale with the length
    const double slots = 2.0 * num_cus;
    const double pairs = (double)((n + V - 1) / V) * (cplx ? 1.0 : 0.5) * Lf;
    ols *= std::ceil(pairs / slots) * slots * (double)V * (cplx ? 1.0 : 2.0) / 67108864.0;
    poly *= (double)n * Lf / 67108864.0;
    if (M == 1) {   // the tile interpolators replace the walk wherever they apply: rounds of one INPUT tile (all phases) per resident workgroup
        if (kind) {
            int Vt = 0;
            const double ms = fir_up_tile_ms(h, L, kind, &Vt);
            const double tiles = (double)((n + Vt - 1) / Vt);
            const double tms = ms * std::ceil(tiles / slots) * slots * (double)Vt * Lf / 67108864.0;
            if (tms < ols) { ols = tms; out.best = 2; }
        }
        if (opt.fir_up_rep && fir_ols_rep_supported(h, L, opt.fir_up_rep)) {
            const double rms = fir_up_rep_ms(h, L) * (double)n * Lf / 67108864.0;
            if (rms < ols) { ols = rms; out.best = 3; }
        }
    }
    out.prefers_ols = ols < poly;
    return out;
}

// ---- the decision ------------------------------------------------------------------------------------------------------------
// the polyphase launcher: the tier it runs, kRouteNone for no output, kRouteRefused where it has no kernel
inline int fir_direct_tier(const FirShape &h, int L, int M, int64_t n_out, int num_cus, const FirRouteOptions &o)
{
    if (n_out <= 0) return kRouteNone;
    if (o.fir_mm && o.fir_bx && fir_bx_supported(h, L, M, n_out, num_cus)) return kRouteBx;
    if (o.fir_mm && fir_mm_supported(h, L, M, n_out)) return kRouteMm;
    return fir_direct_holds(h, L, M) ? kRouteDirect : kRouteRefused;
}

// .filter on one launch
inline FirRoute fir_route_filter(const FirShape &h, const FirCall &c, const FirRouteOptions &o)
{
    FirRoute r;
    if (pick_fir_algo(h, c.n, o) == kFirOls) r.engine = fir_dbl(h) ? kRouteOls64 : kRouteOls;
    else r.engine = fir_direct_tier(h, 1, 1, c.n, c.num_cus, o);
    return r;
}

// the last resort of .dn: the full-rate filter into workspace slot 2 (3 inside a tap-segment call, which holds 2: the planes of a complex IIR
// call, never alive during a FIR call), and a strided copy
inline FirRoute fir_route(const FirShape &h, const FirCall &c, const FirRouteOptions &o);
inline FirRoute fir_route_full_rate(const FirShape &h, const FirCall &c, const FirRouteOptions &o)
{
    FirCall f = c;
    f.n = (c.n / c.M) * c.M; f.L = f.M = 1; f.plain = true;
    FirRoute r = fir_route(h, f, o);
    r.M = c.M; r.copy = kCopyFullRate; r.slot = c.scratch_free ? 2 : 3; r.direct_refused = true;
    return r;
}

// .dn on one launch: long filters with a modest M go through the overlap-save engine with a decimating store, which
// beats Ntaps/M direct taps per kept sample (2^24 complex64, 512 taps, M = 3: 0.163 -> 0.085 ms).  Where the
// matrix-pipe kernel covers the geometry it is the faster one (profiles/r04/fir_dn.txt) except for the long filters of M <= 4.
inline FirRoute fir_route_dn(const FirShape &h, const FirCall &c, const FirRouteOptions &o)
{
    const int M = c.M;
    const int64_t n = c.n;
    FirRoute r;
    r.M = M;
    if (fir_dbl(h)) {  // float64: the decimating overlap-save store beats Ntaps / M direct FP64 taps per kept sample early
        if (M > 1 && pick_fir_algo(h, n, o) == kFirOls && !o.dn_no_ols && h.ntaps / M >= 24) { r.engine = kRouteOls64; r.dec = M; return r; }
        r.engine = fir_direct_tier(h, 1, M, n / M, c.num_cus, o);
        if (r.engine == kRouteRefused && M > 1) {   // (a stride the polyphase kernels' LDS window does not hold: see below)
            if (fir_ols64_supported(h) && !o.dn_no_ols) { r.engine = kRouteOls64; r.dec = M; r.direct_refused = true; return r; }
            return fir_route_full_rate(h, c, o);
        }
        return r;
    }
    bool ols = M > 1 && fir_ols_supported(h) && pick_fir_algo(h, n, o) == kFirOls && !o.dn_no_ols;
    const bool fold = M % 2 == 0 && o.fir_dn_fold;   // even M: the overlap-save tile transforms only the kept outputs back (ols_fold_kernel)
    if (ols) {
        // Which engine (profiles/r05/fir_dn.txt, 2^26 inputs).  The matrix-pipe kernel computes kept outputs only and costs with the taps per kept
        // output u = Ntaps / M; the overlap-save tile costs the same whatever the filter: with the folded inverse transform 0.155 - 0.19 ms
        // (complex64; float32 0.085 - 0.105), with the decimating store (odd M) the plain filter's 0.21 - 0.23.  Measured crossovers: complex64
        // M = 4 from the shortest filter overlap-save takes, M = 2 from u = 96, M = 8, 12, 16 from u = 64, M = 6, 10 from u = 128; float32 from
        // u = 128 (M = 2: 192).  Where the matrix-pipe kernel does not cover the shape (complex taps, lag ranges beyond its 48 blocks) the
        // register sliding-window kernel is the alternative, and cheaper below a few dozen taps per kept output.
        const int kb = h.algo == kFirOls ? -1 : fir_bx_blocks(h, 1, M, o);
        const int u = h.ntaps / M;
        const bool f32 = h.dtype == kFirF32;
        if (kb < 0) ols = true;                                                  // (forced by the caller)
        else if (kb == 0) ols = u >= (f32 ? 64 : 24);
        // (end of round 6, with the matrix-pipe kernel's paired column tiles: complex64 M = 16, u = 64 0.146 against 0.162 ms; float32 M = 8, u = 128 0.093 / 0.098)
        else if (fold) ols = u >= (f32 ? (M == 2 ? 192 : (M == 4 ? 128 : 160)) : (M == 4 ? 0 : (M == 2 ? 96 : (M % 16 == 0 ? 96 : (M % 4 == 0 ? 64 : 128)))));
        else ols = M <= 4 && kb > 12;                                            // (M = 3: complex64 512 taps 0.256 ms against 0.215, float32 0.132 / 0.100)
    }
    // M = 3: the frequency-domain decimator (fir_dn4k.hip: M forward transforms accumulated, ONE inverse per tile of kept outputs) wherever the
    // decimating store would run; even M: the folded inverse is ahead of it everywhere (M = 2, 1024 taps: 0.189 against 0.219 ms; M = 4: 0.174 /
    // 0.237; float32 0.097 / 0.116).  Option fir_dn4k = 2: wherever it applies (A/B timing, tests)
    if (M > 1 && o.fir_dn4k && fir_dn4k_supported(h, M) && n / M >= 2048 &&
        (o.fir_dn4k >= 2 || (ols && !fold && (h.dtype == kFirF32 || h.ntaps > 1536)))) { r.engine = kRouteDn4k; return r; }
    if (ols) { r.engine = kRouteOls; r.dec = M; return r; }
    r.engine = fir_direct_tier(h, 1, M, n / M, c.num_cus, o);
    if (r.engine == kRouteRefused && M > 1) {
        // a stride the polyphase kernels' LDS window does not hold (a few hundred taps and M in the thousands): the decimating
        // overlap-save store takes any M; without that engine, the full-rate filter and a strided copy
        // (that store's index arithmetic is exact up to M = 32768 -- fir_ols_launch checks it --: beyond, the full-rate filter and the strided copy)
        if (fir_ols_supported(h) && !o.dn_no_ols && M <= 32768) { r.engine = kRouteOls; r.dec = M; r.direct_refused = true; return r; }
        return fir_route_full_rate(h, c, o);
    }
    return r;
}

// .up / fused L over M on one launch (L > 1).  The cost model is evaluated at most once.
inline FirRoute fir_route_updn(const FirShape &h, const FirCall &c, const FirRouteOptions &o)
{
    const int L = c.L, M = c.M;
    const int64_t n = c.n;
    const bool dbl = fir_dbl(h);
    FirRoute r;
    r.L = L; r.M = M;
    FirUpModel model;
    bool modelled = false;
    auto prefers_ols = [&]() {
        if (!modelled) { model = fir_up_model(h, L, n, M, c.num_cus, o); modelled = true; }
        return model.prefers_ols;
    };
    const int walk = dbl ? kRouteWalk64 : kRouteWalk;
    if (M == 1) {
        // even L: tiles of the OUTPUT, the zero-stuffed tile's spectrum from its non-zero columns (ols_rep_kernel); option fir_up_rep = 2: wherever it applies
        if (n * L >= 8192 && fir_ols_rep_supported(h, L, o.fir_up_rep) &&
            (o.fir_up_rep >= 2 || (o.fir_up4k < 2 && o.fir_up_ols_min > 0 && prefers_ols() && model.best == 3))) {   // (an engine forced by option stays forced)
            r.engine = kRouteOlsRep;
            return r;
        }
        // one workgroup per input tile, all L phases from ONE forward transform (fir_up4k.hip / fir_up2k.hip); option fir_up4k: 0 never, 2
        // wherever one applies (tests, A/B timing), 1 where the cost model prefers the frequency domain
        if (n >= 2048) {
            const int kind = fir_up_tile_kind(h, L, o);
            if (kind && (o.fir_up4k >= 2 || prefers_ols())) { r.engine = kind == 2 ? kRouteUp2k : kRouteUp4k; return r; }
        }
        if (prefers_ols()) {
            bool paired = dbl ? fir_ols64_up_pairs(h, L, 1, c.y_low, o.fir_up_pair) : fir_ols_up_pairs(h, L, 1, c.y_low, o.fir_up_pair);
            bool rows = c.scratch_free && fir_up_rows(h, L, o, paired) && !(paired && L == 2);   // (one pair is one row: nothing to weave)
            if (rows && paired && L % 2) {   // an odd L in pairs has the strided form only: rows asked for by option win, else the pairs
                if (o.fir_up_rows_min > 0) paired = false; else rows = false;
            }
            // many phases: an output stored between outputs of other phases is a write request of its own, so the phases leave as rows
            // with the plain filter's stores and interleave_launch weaves them (one more pass over the output, still cheaper from L = 6 ... 9 on)
            r.engine = walk; r.paired = paired; r.rows = rows;
            if (rows) r.copy = kCopyWeave;
            return r;
        }
    } else if ((c.scratch_free || (M <= 4096 && o.fir_updn_fused)) && prefers_ols()) {   // long phases: all n L outputs by the walk, every M-th of them kept
        r.engine = walk;
        if (M <= 4096 && o.fir_updn_fused) r.dec = M;   // ... by its store
        else r.copy = kCopyEveryMth;                    // ... or out of scratch
        return r;
    }
    if (fir_needs_parts(h, L)) { r.engine = kRouteParts; r.seg = fir_parts_seg(h, L, M); return r; }
    r.engine = fir_direct_tier(h, L, M, (n * L) / M, c.num_cus, o);
    if (r.engine == kRouteRefused && M > 1 && M <= 4096 && L <= 64 && o.fir_up_ols_min != 0 && (dbl ? fir_ols64_up_supported(h, L) : fir_ols_up_supported(h, L))) {
        r.engine = walk; r.dec = M; r.direct_refused = true;   // (a stride the polyphase kernels' LDS window does not hold)
    }
    return r;
}

// one launch (a tap segment, or a call that needs none): no head, no segments
inline FirRoute fir_route_single(const FirShape &h, const FirCall &c, const FirRouteOptions &o)
{
    if (c.plain) return fir_route_filter(h, c, o);
    return c.L == 1 ? fir_route_dn(h, c, o) : fir_route_updn(h, c, o);
}

// The route of a call.  A filter longer than one launch takes (fir_needs_parts) runs as tap segments, y[m] = sum_s (b_s * x)[m - s seg]; a
// .filter call from rest over fewer samples than taps runs on a head of the filter.
inline FirRoute fir_route(const FirShape &h_in, const FirCall &c, const FirRouteOptions &o)
{
    FirShape h = h_in;
    const int head = c.plain && c.n_hist == 0 && c.n < h.ntaps ? fir_head_taps(h.ntaps, c.n) : 0;
    if (head) h.ntaps = head;
    FirRoute r;
    if (c.L == 1 && fir_needs_parts(h)) {   // (.up / L over M: behind the frequency-domain engines, which take longer phases -- fir_route_updn)
        r.engine = kRouteParts; r.M = c.M; r.seg = fir_parts_seg(h, 1, c.M);
    } else {
        r = fir_route_single(h, c, o);
    }
    if (r.engine == kRouteParts && !(fir_parts_seg_ok(h, r.seg, c.L) && fir_parts_history_ok(h, r.seg, c.L, c.M, c.n_hist))) r.engine = kRouteRefused;
    if (head) r.head = head;
    return r;
}

// ---- the engines a call notes (skdsp_debug_path) -------------------------------------------------------------------------------
inline const char *fir_engine_name(int engine)
{
    switch (engine) {
    case kRouteBx: return "fir_bx";
    case kRouteMm: return "fir_mm";
    case kRouteDirect: case kRouteRefused: return "fir_direct";
    case kRouteOls: return "fir_ols";
    case kRouteOls64: return "fir_ols64";
    case kRouteDn4k: return "fir_dn4k";
    case kRouteUp4k: return "fir_up4k";
    case kRouteUp2k: return "fir_up2k";
    case kRouteOlsRep: return "fir_ols_rep";
    case kRouteWalk: return "fir_ols_up";
    case kRouteWalk64: return "fir_ols64_up";
    default: return "";
    }
}
// note_path's rule: a name equal to the last one is not repeated
inline void fir_note_engine(std::vector<std::string> &path, const char *name)
{
    if (*name && (path.empty() || path.back() != name)) path.push_back(name);
}
// the names the execution of `r` notes, in order; a tap-segment call: the concatenation over its segments, each routed on its own shape
inline std::vector<std::string> fir_route_engines(const FirRoute &r, const FirShape &h_in, const FirCall &c, const FirRouteOptions &o)
{
    std::vector<std::string> path;
    FirShape h = h_in;
    if (r.head) h.ntaps = r.head;
    if (r.seg == 0) {
        if (r.direct_refused) fir_note_engine(path, fir_engine_name(kRouteDirect));
        fir_note_engine(path, fir_engine_name(r.engine));
        return path;
    }
    if (r.engine == kRouteRefused) return path;   // (the segment or the history rule: refused before any launch)
    const int64_t n = c.L == 1 ? (c.n / c.M) * c.M : c.n;
    for (int si = 0; si < fir_parts_count(h, r.seg); ++si) {
        FirSegment s;
        if (!fir_parts_segment(h, r.seg, si, n, c.n_hist, c.L, c.M, &s)) break;
        const FirShape p{h.dtype, s.taps, h.taps_complex, h.algo};
        const FirCall cs{s.n, s.n_hist, c.L, c.M, c.L == 1 && c.M == 1, si == 0 ? c.y_low : 0u, false, c.num_cus};
        const FirRoute rs = fir_route_single(p, cs, o);
        for (const std::string &e : fir_route_engines(rs, p, cs, o)) fir_note_engine(path, e.c_str());
        if (rs.engine == kRouteRefused) break;
    }
    return path;
}

}  // namespace skdsp
