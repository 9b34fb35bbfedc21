// fir_api.hip -- FIR dispatch behind the extern "C" boundary (see include/skdsp.h): the measured cost models that pick an
// engine per call, tap segments, heads, rows, and the FIR entry points.
#include "api_internal.hpp"
#include <cmath>
#include <numeric>

namespace skdsp {

// FIR .filter algorithm choice.  OLS needs complex64; it wins once direct form stops
// being HBM-bound (2*P FMA per c64 sample on the VALU vs ~120 flop in the FFT domain).
static int pick_fir_algo(const FirHandle *h, int64_t n)
{
    int algo = opt().fir_algo != SKDSP_FIR_AUTO ? opt().fir_algo : h->algo;
    const bool ols64 = fir_ols64_supported(h);
    if (algo == SKDSP_FIR_OLS && !fir_ols_supported(h) && !ols64) algo = SKDSP_FIR_DIRECT;
    if (algo != SKDSP_FIR_AUTO) return algo;
    // float64 signals: the direct form costs 2 (4 for complex taps) FP64 FMA per tap and real sample; the float64
    // overlap-save tile is flat in the tap count (measured crossovers at 2^26 samples: see DESIGN.md 4.2, LABNOTES.md)
    if (ols64) return h->ntaps >= (h->dtype == SKDSP_C128 ? 24 : 128) && n >= 8192 ? SKDSP_FIR_OLS : SKDSP_FIR_DIRECT;
    // measured crossover at 2^26 samples (tools/time_fir_filter.py, profiles/r04/fir_filter.txt): the matrix-pipe kernel (real taps, fp16 pieces)
    // stays ahead of overlap-save up to 6 lag blocks for complex64 (0.215 vs 0.229 ms at 145 taps; 0.221 vs 0.227 at 160; 0.241 vs 0.227 at 192)
    // and for float32 (0.109 vs 0.125 ms at 145 taps; 0.125 vs 0.126 at 192; 0.133 vs 0.122 at 224)
    const int ols_from = h->taps_complex ? 48 : (h->dtype == SKDSP_C64 ? 177 : 193);
    if (fir_ols_supported(h) && h->ntaps >= ols_from && n >= 4096) return SKDSP_FIR_OLS;
    return SKDSP_FIR_DIRECT;
}

int fir_algo_for(const FirHandle *h, int64_t n) { return pick_fir_algo(h, n); }

// .dn: long filters with a modest M go through the overlap-save engine with a decimating store, which
// beats Ntaps/M direct taps per kept sample (2^24 complex64, 512 taps, M = 3: 0.163 -> 0.085 ms).  Where the
// matrix-pipe kernel covers the geometry it is the faster one (profiles/r04/fir_dn.txt) except for the long filters of M <= 4: fir_dn_any.
// ---- tap partitioning: filters longer than one launch takes ------------------------------------------------------
// The reference accepts any tap count (lfilter(b,[1],x), multirate_helper.py:108).  One launch takes up to 4097 taps in
// the overlap-save engine (float32 / complex64) and a few thousand in the float64 direct-form kernels (LDS window); a
// longer b is cut into segments of `seg` taps,  y[m] = sum_s (b_s * x)[m - s seg]:  segment s is an ordinary filter
// launch over the input shortened by its delay (with as much of the caller's history as it can still see), and its
// result is added onto y from output s seg on.  For .dn the segment length is a multiple of M, so every partial
// result keeps decimation phase 0.
// A handle over taps [t0, t0 + cnt) of `h` on slot `slot`: the ONE place that copies a FIR handle's fields (tap segments, the heads of short calls,
// the per-slot clones of the multi-GPU host path), so that a field added to FirHandle cannot be forgotten in one of them.
static FirHandle *fir_derive(const FirHandle *h, int t0, int cnt, int slot)
{
    const int comp = h->taps_complex ? 2 : 1;
    FirHandle *d = new FirHandle();
    d->kind = H_FIR; d->dtype = h->dtype; d->slot = slot; d->taps_complex = h->taps_complex; d->algo = h->algo; d->wide_out = h->wide_out;
    d->ntaps = cnt;
    d->taps_host.assign(h->taps_host.begin() + (size_t)t0 * comp, h->taps_host.begin() + (size_t)(t0 + cnt) * comp);
    return d;
}

static int fir_part_len(const FirHandle *h)
{
    return dtype_double(h->dtype) ? 2048 : 4096;
}
static bool fir_needs_parts(const FirHandle *h, int L = 1)
{
    // per launch: 4097 taps (float32 overlap-save / direct) or 2049 (float64); an interpolator holds ceil(Ntaps / L) per phase
    const int per_phase = (h->ntaps + L - 1) / L;
    return per_phase > (dtype_double(h->dtype) ? 2049 : 4097);
}
static int fir_dn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev, bool scratch_free = true);
static int fir_updn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev, bool scratch_free = true);
static int fir_filter_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev);
static int ols_launch_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev, int dec = 1);
// y[j] = L sum_t b[(j M mod L) + L t] x[(j M div L) - t] with b cut into segments of `seg` taps, seg a multiple of lcm(L, M):
// segment s delays the up-rate signal by s seg samples = s seg / L input samples = s seg / M outputs, so it is the same
// operation over the input shortened by s seg / L samples, added onto y from output s seg / M on.  With history in front
// of x the segment starts d input samples early (d a multiple of M / gcd(L, M): whole outputs) and lands d L / M outputs earlier.
static int fir_parts_run(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev)
{
    const int g = std::gcd(L, M), lcm = L / g * M, q = M / g;
    const int seg = std::max(fir_part_len(h) * L / lcm, 1) * lcm;   // <= fir_part_len taps per phase
    if (h->part_seg != seg) {
        for (FirHandle *p : h->parts) delete p;
        h->parts.clear();
        for (int t0 = 0; t0 < h->ntaps; t0 += seg) h->parts.push_back(fir_derive(h, t0, std::min(seg, h->ntaps - t0), h->slot));
        h->part_seg = seg;
    }
    for (FirHandle *p : h->parts) p->algo = h->algo;   // (skdsp_fir_set_algo after the parts were made)
    // A segment may start inside the history only by whole output periods (q inputs).  A history that covers a segment's
    // delay is used in full; a shorter one is used up to a multiple of q -- if it is not one itself, the samples
    // x[-n_hist .. -d-1] would be dropped from the outputs just below that segment's first one, so such a call is refused
    // (the host pipeline and the sharded path always hand over a history that is complete or a multiple of q).
    {
        const int64_t last_delay = (int64_t)(h->parts.size() - 1) * seg / L;
        SK_CHECK(q == 1 || n_hist >= last_delay || n_hist % q == 0, SKDSP_ERR_UNSUPPORTED,
                 "fir: %d taps run as %d tap segments; with L/M = %d/%d a partial history (n_hist = %lld < %lld) must be a multiple of %d samples",
                 h->ntaps, (int)h->parts.size(), L, M, (long long)n_hist, (long long)last_delay, q);
    }
    const size_t esz = dtype_size(h->dtype);
    const int scal = dtype_complex(h->dtype) ? 2 : 1;
    hipStream_t s = ctx().stream;
    const int64_t n_out = (n * L) / M;
    void *tmp = nullptr;
    int rc = ws_reserve(2, (size_t)(n_out + 1) * esz + 256, &tmp);
    if (rc) return rc;
    for (size_t si = 0; si < h->parts.size(); ++si) {
        FirHandle *p = h->parts[si];
        const int64_t delay_in = (int64_t)si * seg / L, delay_out = (int64_t)si * seg / M;
        const int64_t d = (std::min(n_hist, delay_in) / q) * q;       // how far this segment starts inside the history
        const int64_t n_s = n - delay_in + d;
        const int64_t off = delay_out - d * L / M;                    // first output this segment contributes to
        const int64_t cnt = std::min((n_s * L) / M, n_out - off);
        if (n_s <= 0 || cnt <= 0) break;
        const char *xs = (const char *)x_dev - (size_t)d * esz;
        void *dst = si == 0 ? y_dev : tmp;
        if (L == 1 && M == 1)
            rc = fir_algo_for(p, n_s) == SKDSP_FIR_OLS ? ols_launch_any(p, xs, n_s, n_hist - d, dst)
                                                        : fir_direct_launch(p, xs, n_s, n_hist - d, 1, 1, n_s, dst, s);
        else if (L == 1)
            rc = fir_dn_any(p, xs, n_s, n_hist - d, M, dst, false);   // (workspace slot 2 is `tmp` -- possibly `dst` -- here)
        else
            rc = fir_updn_any(p, xs, n_s, n_hist - d, L, M, dst, false);   // (workspace slot 2 is `tmp` here: no scratch-using forms; writes (n_s L) / M <= n_out outputs)
        if (rc) return rc;
        if (si > 0 && (rc = accumulate_launch((char *)y_dev + (size_t)off * esz, tmp, cnt * scal, dtype_double(h->dtype), s))) return rc;
    }
    return SKDSP_OK;
}

static int ols_launch_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev, int dec)
{
    if (dtype_double(h->dtype)) return fir_ols64_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, dec);
    return fir_ols_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, dec);
}

// the last resort of .dn: the full-rate filter into workspace slot `full_slot`, and a strided copy
static int fir_dn_full_rate(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev, int full_slot)
{
    void *full = nullptr;
    const int64_t nk = (n / M) * M;
    int rc = ws_reserve(full_slot, (size_t)nk * dtype_size(h->dtype) + 256, &full);
    if (rc) return rc;
    if ((rc = fir_filter_any(h, x_dev, nk, n_hist, full))) return rc;
    return downsample_launch(full, nk, M, 0, h->dtype, y_dev, ctx().stream);
}

// scratch_free: workspace slot 2 may hold the full-rate result of the last-resort path (false inside fir_parts_run, which holds it: slot 3 then --
// the planes of a complex IIR call, never alive during a FIR call)
static int fir_dn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev, bool scratch_free)
{
    const int full_slot = scratch_free ? 2 : 3;
    if (fir_needs_parts(h)) return fir_parts_run(h, x_dev, (n / M) * M, n_hist, 1, M, y_dev);
    if (dtype_double(h->dtype)) {  // float64: the decimating overlap-save store beats Ntaps / M direct FP64 taps per kept sample early
        if (M > 1 && pick_fir_algo(h, n) == SKDSP_FIR_OLS && !opt().dn_no_ols && h->ntaps / M >= 24)
            return fir_ols64_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, M);
        int rc = fir_direct_launch(h, x_dev, n, n_hist, 1, M, n / M, y_dev, ctx().stream);
        if (rc == SKDSP_ERR_UNSUPPORTED && M > 1) {   // (a stride the polyphase kernels' LDS window does not hold: see below)
            if (fir_ols64_supported(h) && !opt().dn_no_ols) return fir_ols64_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, M);
            return fir_dn_full_rate(h, x_dev, n, n_hist, M, y_dev, full_slot);
        }
        return rc;
    }
    bool ols = M > 1 && fir_ols_supported(h) && pick_fir_algo(h, n) == SKDSP_FIR_OLS && !opt().dn_no_ols;
    const bool fold = M % 2 == 0 && opt().fir_dn_fold;   // even M: the overlap-save tile transforms only the kept outputs back (ols_fold_kernel)
    if (ols) {
        // Which engine (profiles/r05/fir_dn.txt, 2^26 inputs).  The matrix-pipe kernel computes kept outputs only and costs with the taps per kept
        // output u = Ntaps / M; the overlap-save tile costs the same whatever the filter: with the folded inverse transform 0.155 - 0.19 ms
        // (complex64; float32 0.085 - 0.105), with the decimating store (odd M) the plain filter's 0.21 - 0.23.  Measured crossovers: complex64
        // M = 4 from the shortest filter overlap-save takes, M = 2 from u = 96, M = 8, 12, 16 from u = 64, M = 6, 10 from u = 128; float32 from
        // u = 128 (M = 2: 192).  Where the matrix-pipe kernel does not cover the shape (complex taps, lag ranges beyond its 48 blocks) the
        // register sliding-window kernel is the alternative, and cheaper below a few dozen taps per kept output.
        const int kb = h->algo == SKDSP_FIR_OLS ? -1 : fir_bx_blocks(h, 1, M);
        const int u = h->ntaps / M;
        const bool f32 = h->dtype == SKDSP_F32;
        if (kb < 0) ols = true;                                                  // (forced by the caller)
        else if (kb == 0) ols = u >= (f32 ? 64 : 24);
        // (end of round 6, with the matrix-pipe kernel's paired column tiles: complex64 M = 16, u = 64 0.146 against 0.162 ms; float32 M = 8, u = 128 0.093 / 0.098)
        else if (fold) ols = u >= (f32 ? (M == 2 ? 192 : (M == 4 ? 128 : 160)) : (M == 4 ? 0 : (M == 2 ? 96 : (M % 16 == 0 ? 96 : (M % 4 == 0 ? 64 : 128)))));
        else ols = M <= 4 && kb > 12;                                            // (M = 3: complex64 512 taps 0.256 ms against 0.215, float32 0.132 / 0.100)
    }
    // M = 3: the frequency-domain decimator (fir_dn4k.hip: M forward transforms accumulated, ONE inverse per tile of kept outputs) wherever the
    // decimating store would run; even M: the folded inverse is ahead of it everywhere (M = 2, 1024 taps: 0.189 against 0.219 ms; M = 4: 0.174 /
    // 0.237; float32 0.097 / 0.116).  Option fir_dn4k = 2: wherever it applies (A/B timing, tests)
    if (M > 1 && opt().fir_dn4k && fir_dn4k_supported(h, M) && n / M >= 2048 &&
        (opt().fir_dn4k >= 2 || (ols && !fold && (h->dtype == SKDSP_F32 || h->ntaps > 1536))))
        return fir_dn4k_launch(h, x_dev, n, n_hist, M, y_dev, ctx().stream);
    if (ols) return fir_ols_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, M);
    int rc = fir_direct_launch(h, x_dev, n, n_hist, 1, M, n / M, y_dev, ctx().stream);
    if (rc == SKDSP_ERR_UNSUPPORTED && M > 1) {
        // a stride the polyphase kernels' LDS window does not hold (a few hundred taps and M in the thousands): the decimating
        // overlap-save store takes any M; without that engine, the full-rate filter and a strided copy
        // (that store's index arithmetic is exact up to M = 32768 -- fir_ols_launch checks it --: beyond, the full-rate filter and the strided copy)
        if (fir_ols_supported(h) && !opt().dn_no_ols && M <= 32768) return fir_ols_launch(h, x_dev, n, n_hist, y_dev, ctx().stream, M);
        return fir_dn_full_rate(h, x_dev, n, n_hist, M, y_dev, full_slot);
    }
    return rc;
}

// .up / fused L over M: one polyphase launch, or tap segments when a phase holds more taps than a launch takes
// multirate_FIR.up: polyphase kernels or the overlap-save walk over (tile, phase) pairs (fir_ols.hip)?  Both are timed models of this
// board at 2^26 outputs (tools/time_fir_up.py; ms), scaled to the call: the polyphase kernels cost per tap of a phase -- little where the
// matrix-pipe kernel covers the shape, 3-4x that where it does not -- the walk costs per (tile, phase) pair whatever the phase length,
// plus what its stride-L stores cost, and runs in rounds of one pair per resident workgroup.
// multirate_FIR.up through the overlap-save walk: from which L on the phases leave as rows of scratch and a second kernel weaves them
// (measured crossovers of profiles/r03/fir_up.txt -- the walk serves float64 and > 1025 taps per phase today; 16-byte samples never: their strided stores are full-width requests already)
static bool fir_up_rows(const FirHandle *h, int L, bool paired = false)
{
    const int o = opt().fir_up_rows_min;
    if (o == 0) return false;
    if (o > 0) return L >= o;
    if (paired) return !dtype_double(h->dtype) && L % 2 == 0 && L / 2 >= 7;   // (8-byte pairs: the complex64 crossover, in phases; 16-byte pairs never;
                                                                              //  odd L in pairs: the strided form only)
    switch (h->dtype) {
    case SKDSP_F32: return L >= 9;
    case SKDSP_C64: return L >= 7;
    case SKDSP_F64: return L >= 6;
    default: return false;
    }
}

// The one-workgroup-per-input-tile interpolators (fir_up4k.hip: up to four passes per thread; fir_up2k.hip: all passes of a row per
// thread): which one a call takes (0: none applies), and what it costs in ms per 2^26 outputs on this board (round-4 timings,
// tools/time_up4k.py; the measured shapes had 3 - 6 % of their tile in the overlap, so the figure is scaled to the call's overlap).
static int fir_up_tile_kind(const FirHandle *h, int L)
{
    if (dtype_double(h->dtype) || !opt().fir_up4k) return 0;
    const int passes = h->dtype == SKDSP_F32 ? (L + 1) / 2 : L;   // (float32: two phases per complex pass)
    // float32, L = 2: one pass -- the walk's pair form IS the plain filter's 8192-point tile with an 8-byte store, and stays ahead of the
    // 4096-point tile (512 / 1024 taps per phase: 0.117 / 0.125 ms against 0.126 / 0.140)
    if (passes == 1 && opt().fir_up4k < 2) return 0;
    if (opt().fir_up2k && fir_up2k_supported(h, L) && (opt().fir_up2k >= 2 || passes > 4)) return 2;
    return fir_up4k_supported(h, L) ? 4 : 0;
}
static double fir_up_tile_ms(const FirHandle *h, int L, int kind, int *V_out)
{
    const int T = (h->ntaps + L - 1) / L;
    const int passes = h->dtype == SKDSP_F32 ? (L + 1) / 2 : L;
    const bool cplx = h->dtype == SKDSP_C64;
    double ms;
    int N, ov;
    if (kind == 4) {   // 4096-point tile, groups of four passes: one group is one burst per row, more are pieces written far apart
        N = 4096; ov = std::max(256, (T - 1 + 255) / 256 * 256);
        // (one group: the forward transform is shared by `passes` inverse ones -- 0.2025 / 0.199 / 0.187 ms at 2 / 3 / 4 complex64 passes,
        // 0.1225 / 0.0946 / 0.105 / 0.096 at 1 .. 4 float32 passes, profiles/r04/fir_up.txt)
        static const double c4[5] = {0.0, 0.26, 0.2025, 0.199, 0.187}, f4[5] = {0.0, 0.1225, 0.0946, 0.105, 0.096};
        ms = cplx ? (passes <= 4 ? c4[passes] : 0.30 + 0.012 * std::min(passes, 12)) : (passes <= 4 ? f4[passes] : 0.10 + 0.005 * std::min(passes, 12));
        ms *= (4096.0 - 256.0) / 4096.0;
    } else {           // 2048-point tile, up to twelve passes per thread
        N = 2048; ov = std::max(64, (T - 1 + 63) / 64 * 64);
        if (passes <= 12) ms = cplx ? 0.19 + 0.0025 * passes : 0.085 + 0.0035 * passes;
        else ms = cplx ? 0.36 : 0.16;
        if (passes % 2) ms *= 1.07;   // (an odd row: every lane stores its own pieces)
        ms *= (2048.0 - 64.0) / 2048.0;
    }
    *V_out = N - ov;
    return ms * (double)N / (double)(N - ov);
}

// multirate_FIR.up, even L, on tiles of the OUTPUT (fir_ols.hip: ols_rep_kernel): ms per 2^26 outputs (round-5 timings, profiles/r05/fir_up.txt: the plain
// filter's tile with a quarter of its forward transform and 1 / L of its loads; the overlap is that of the WHOLE filter at the high rate)
static double fir_up_rep_ms(const FirHandle *h, int L)
{
    const int ov = std::max(512, (h->ntaps - 1 + 511) / 512 * 512);
    const bool cplx = h->dtype == SKDSP_C64;
    const bool pow2 = (L & (L - 1)) == 0 && L <= 16;   // (else the decimated grid is itself zero-stuffed: the guarded loader, 4-byte samples feel it)
    const double base = cplx ? (L == 2 ? 0.161 : 0.152) : (L == 2 ? 0.087 : (L == 4 ? 0.083 : 0.0885)) * (pow2 ? 1.0 : 1.18);
    return base * 8192.0 / (8192.0 - ov);
}

// best: which frequency-domain engine the model found cheapest (1 the walk over (tile, phase) pairs, 2 an input-tile interpolator, 3 the output-tile one)
static bool fir_up_prefers_ols(const FirHandle *h, int L, int64_t n, int M = 1, int *best = nullptr)
{
    if (best) *best = 1;
    const int T = (h->ntaps + L - 1) / L;
    const int floor_t = opt().fir_up_ols_min;   // < 0: wherever supported from -floor_t taps per phase on, no cost model (tests, A/B timing)
    const bool dbl = dtype_double(h->dtype);
    int floor_eff = std::abs(floor_t);   // (many phases: the polyphase kernels lose their reuse early -- let the cost model see shorter phases too)
    if (floor_t > 0 && L > 64) floor_eff = std::max(8, floor_t / 8);
    else if (floor_t > 0 && L > 16) floor_eff = std::max(8, floor_t / 4);
    if (M == 1 && floor_t > 0 && fir_up_tile_kind(h, L)) floor_eff = std::min(floor_eff, 24);   // (the tile interpolators cross over with the polyphase kernels at short phases already)
    if (floor_t == 0 || T < floor_eff || n < 8192 || !(dbl ? fir_ols64_up_supported(h, L) : fir_ols_up_supported(h, L))) return false;
    if (M > 1 && L > 64) return false;   // (the every-M-th store's exact-division range; the scratch + copy form is not worth it there)
    if (floor_t < 0) return true;
    if ((opt().fir_algo != SKDSP_FIR_AUTO ? opt().fir_algo : h->algo) == SKDSP_FIR_DIRECT) return false;
    if (fir_needs_parts(h, L)) return true;   // (longer than one polyphase launch takes)
    // all figures: ms per 2^26 up-rate samples on this board (the walk and the float64 kernels: profiles/r03/fir_up.txt, fir_updn.txt; the matrix-pipe and tile kernels: profiles/r04)
    const double Lf = (double)L;
    const bool cplx = dtype_complex(h->dtype);
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
        const int bx_kb = fir_bx_blocks(h, L, M, &bx_rt);   // (the matrix-pipe polyphase kernel covers the shape: its time goes with its 32-lag blocks)
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
    if (M == 1 && fir_up_rows(h, L)) ols = std::min(ols, dbl ? 0.45 : (cplx ? 0.45 : 0.245));   // (rows + weave: whatever L is)
    if (M == 1 && !dbl && fir_ols_up_pairs(h, L, 1, nullptr))   // float32, even L: L / 2 complex passes per tile of real input, 8-byte outputs
        ols = std::min(0.11 + 0.007 * Lf, 0.235);
    if (M == 1 && dbl && fir_ols64_up_pairs(h, L, 1, nullptr))   // float64 likewise, 16-byte outputs
        ols = 0.25 + 0.005 * std::min(Lf, 16.0);
    if (M > 1) {   // L / M: the polyphase kernels compute the kept outputs only; the walk computes all and stores (or copies) every M-th
        poly /= (double)M;
        if (M <= 4096 && opt().fir_updn_fused) ols = base + (ols - base) / (double)M;
        else ols += copy;
    }
    // the walk runs in rounds of one (tile, phase) pair per resident workgroup; the polyphase kernels scale with the length
    const double slots = 2.0 * ctx().num_cus;
    const double pairs = (double)((n + V - 1) / V) * (cplx ? 1.0 : 0.5) * Lf;
    ols *= std::ceil(pairs / slots) * slots * (double)V * (cplx ? 1.0 : 2.0) / 67108864.0;
    poly *= (double)n * Lf / 67108864.0;
    if (M == 1) {   // the tile interpolators replace the walk wherever they apply: rounds of one INPUT tile (all phases) per resident workgroup
        const int kind = fir_up_tile_kind(h, L);
        if (kind) {
            int Vt = 0;
            const double ms = fir_up_tile_ms(h, L, kind, &Vt);
            const double tiles = (double)((n + Vt - 1) / Vt);
            const double tms = ms * std::ceil(tiles / slots) * slots * (double)Vt * Lf / 67108864.0;
            if (tms < ols) { ols = tms; if (best) *best = 2; }
        }
        if (opt().fir_up_rep && fir_ols_rep_supported(h, L)) {
            const double rms = fir_up_rep_ms(h, L) * (double)n * Lf / 67108864.0;
            if (rms < ols) { ols = rms; if (best) *best = 3; }
        }
    }
    return ols < poly;
}

// scratch_free: workspace slot 2 may be used (rows of the .up walk, the unfused L / M copy); false inside fir_parts_run, which holds it
static int fir_updn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev, bool scratch_free)
{
    if (L == 1) return fir_dn_any(h, x_dev, n, n_hist, M, y_dev);
    const bool dbl = dtype_double(h->dtype);
    auto walk = [&](void *out, int dec, int64_t pitch = 0, int paired = 0) {
        return dbl ? fir_ols64_up_launch(h, x_dev, n, n_hist, L, out, ctx().stream, dec, pitch, paired)
                   : fir_ols_up_launch(h, x_dev, n, n_hist, L, out, ctx().stream, dec, pitch, paired);
    };
    // even L: tiles of the OUTPUT, the zero-stuffed tile's spectrum from its non-zero columns (ols_rep_kernel); option fir_up_rep = 2: wherever it applies
    if (M == 1 && n * L >= 8192 && fir_ols_rep_supported(h, L)) {
        int best = 0;
        if (opt().fir_up_rep >= 2 || (opt().fir_up4k < 2 && opt().fir_up_ols_min > 0 && fir_up_prefers_ols(h, L, n, 1, &best) && best == 3))   // (an engine forced by option stays forced)
            return fir_ols_rep_launch(h, x_dev, n, n_hist, L, y_dev, ctx().stream);
    }
    // one workgroup per input tile, all L phases from ONE forward transform (fir_up4k.hip / fir_up2k.hip); option fir_up4k: 0 never, 2
    // wherever one applies (tests, A/B timing), 1 where the cost model above prefers the frequency domain
    if (M == 1 && n >= 2048) {
        const int kind = fir_up_tile_kind(h, L);
        if (kind && (opt().fir_up4k >= 2 || fir_up_prefers_ols(h, L, n)))
            return kind == 2 ? fir_up2k_launch(h, x_dev, n, n_hist, L, y_dev, ctx().stream) : fir_up4k_launch(h, x_dev, n, n_hist, L, y_dev, ctx().stream);
    }
    if (M == 1 && fir_up_prefers_ols(h, L, n)) {
        bool paired = dbl ? fir_ols64_up_pairs(h, L, 1, y_dev) : fir_ols_up_pairs(h, L, 1, y_dev);
        bool rows = scratch_free && fir_up_rows(h, L, paired) && !(paired && L == 2);   // (one pair is one row: nothing to weave)
        if (rows && paired && L % 2) {   // an odd L in pairs has the strided form only: rows asked for by option win, else the pairs
            if (opt().fir_up_rows_min > 0) paired = false; else rows = false;
        }
        if (rows) {
            // many phases: an output stored between outputs of other phases is a write request of its own, so the phases leave as rows
            // with the plain filter's stores and interleave_launch weaves them (one more pass over the output, still cheaper from L = 6 ... 9 on)
            const int rows_n = paired ? L / 2 : L;
            const int row_dtype = paired ? (dbl ? SKDSP_C128 : SKDSP_C64) : h->dtype;
            const int64_t pitch = (int64_t)round_up((size_t)n, 64);
            void *rows = nullptr;
            int rc = ws_reserve(2, (size_t)pitch * rows_n * dtype_size(row_dtype) + 256, &rows);
            if (rc) return rc;
            if ((rc = walk(rows, 1, pitch, paired))) return rc;
            return interleave_launch(rows, n, rows_n, pitch, row_dtype, y_dev, ctx().stream);
        }
        return walk(y_dev, 1, 0, paired);
    }
    if (M > 1 && (scratch_free || (M <= 4096 && opt().fir_updn_fused)) && fir_up_prefers_ols(h, L, n, M)) {   // long phases: all n L outputs by the walk, every M-th of them kept
        if (M <= 4096 && opt().fir_updn_fused) return walk(y_dev, M);   // ... by its store
        void *full = nullptr;                                           // ... or out of scratch
        int rc = ws_reserve(2, (size_t)n * L * dtype_size(h->dtype) + 256, &full);
        if (rc) return rc;
        if ((rc = walk(full, 1))) return rc;
        return downsample_launch(full, n * L, M, 0, h->dtype, y_dev, ctx().stream);
    }
    if (fir_needs_parts(h, L)) return fir_parts_run(h, x_dev, n, n_hist, L, M, y_dev);
    int rc = fir_direct_launch(h, x_dev, n, n_hist, L, M, (n * L) / M, y_dev, ctx().stream);
    if (rc == SKDSP_ERR_UNSUPPORTED && M > 1 && M <= 4096 && L <= 64 && opt().fir_up_ols_min != 0 &&
        (dtype_double(h->dtype) ? fir_ols64_up_supported(h, L) : fir_ols_up_supported(h, L)))
        return walk(y_dev, M);   // (a stride the polyphase kernels' LDS window does not hold)
    return rc;
}

// A call from rest over n < Ntaps samples computes y[m] = sum_(k <= m) b[k] x[m - k], m < n: taps b[n ...] are never reached.  It runs on a
// copy of the filter cut to the next power of two >= n (at most log2(Ntaps) copies per handle) -- the same outputs exactly, less work, and
// the rounding of a float32 engine (a few 1e-8 of sum |b| max |x|: the FFT engines round against the WHOLE filter) shrinks with the taps
// that matter.  (Found by the differential test at north_star's bound without its former factor 2: 17 rows of 100 samples through a
// 1024-tap low-pass, whose first 100 taps are its tail -- 1.7e-6 of the tiny start-up transient before, far inside 1e-6 after.)
static FirHandle *fir_head(FirHandle *h, int64_t n)
{
    if (n >= h->ntaps || n < 1) return h;
    int keep = 1;
    while (keep < n) keep <<= 1;
    if (keep >= h->ntaps) return h;
    for (FirHandle *t : h->heads)
        if (t->ntaps == keep) { t->algo = h->algo; return t; }
    // (at most log2(Ntaps) <= 13 heads per handle -- one per power of two below the tap count -- each with the tables of the engines it has run on: they
    // live as long as the handle)
    FirHandle *t = fir_derive(h, 0, keep, h->slot);
    h->heads.push_back(t);
    return t;
}

static int fir_filter_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev)
{
    if (n_hist == 0 && n < h->ntaps) h = fir_head(h, n);
    if (fir_needs_parts(h)) return fir_parts_run(h, x_dev, n, n_hist, 1, 1, y_dev);
    if (pick_fir_algo(h, n) == SKDSP_FIR_OLS) return ols_launch_any(h, x_dev, n, n_hist, y_dev);
    return fir_direct_launch(h, x_dev, n, n_hist, 1, 1, n, y_dev, ctx().stream);
}

}  // namespace skdsp

using namespace skdsp;

extern "C" {

// ------------------------------------------------------------------------ FIR
int skdsp_fir_create(const void *taps, int ntaps, int taps_complex, int dtype, skdsp_handle *out)
{
    API_BEGIN;
    SK_CHECK(out, SKDSP_ERR_BADARG, "fir_create: null out");
    SK_CHECK(taps && ntaps >= 1, SKDSP_ERR_BADARG, "fir_create: need at least one tap");
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "fir_create: bad dtype %d", dtype);
    SK_CHECK(!(taps_complex && !dtype_complex(dtype)), SKDSP_ERR_BADARG,
             "fir_create: complex taps need a complex signal dtype");
    std::unique_ptr<FirHandle> h(new FirHandle());
    h->kind = H_FIR;
    h->dtype = dtype;
    h->ntaps = ntaps;
    h->taps_complex = taps_complex != 0;
    const int comp = taps_complex ? 2 : 1;
    h->taps_host.assign((const double *)taps, (const double *)taps + (size_t)ntaps * comp);
    *out = h.release();
    return SKDSP_OK;
}

int skdsp_fir_set_algo(skdsp_handle hh, int algo)
{
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_set_algo: not a FIR handle");
    SK_CHECK(algo >= SKDSP_FIR_AUTO && algo <= SKDSP_FIR_OLS, SKDSP_ERR_BADARG, "fir_set_algo: bad algo %d", algo);
    h->algo = algo;
    return SKDSP_OK;
}

int skdsp_fir_get_algo(skdsp_handle hh, int64_t n, int *algo_used)
{
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h && algo_used, SKDSP_ERR_BADARG, "fir_get_algo: bad arguments");
    *algo_used = pick_fir_algo(h, n);
    return SKDSP_OK;
}

int skdsp_fir_filter_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter: not a FIR handle");
    SK_CHECK(n >= 0 && n_hist >= 0, SKDSP_ERR_BADARG, "fir_filter: negative length");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_filter_any(h, x_dev, n, n_hist, y_dev);
}

int skdsp_fir_up_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_up: not a FIR handle");
    SK_CHECK(L >= 1, SKDSP_ERR_BADARG, "fir_up: L must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_updn_any(h, x_dev, n, n_hist, L, 1, y_dev);
}

int skdsp_fir_dn_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_dn: not a FIR handle");
    SK_CHECK(M >= 1, SKDSP_ERR_BADARG, "fir_dn: M must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_dn_any(h, x_dev, n, n_hist, M, y_dev);
}

int skdsp_fir_updn_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_updn: not a FIR handle");
    SK_CHECK(L >= 1 && M >= 1, SKDSP_ERR_BADARG, "fir_updn: L, M must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_updn_any(h, x_dev, n, n_hist, L, M, y_dev);
}

// one chunk of a long host vector (run_pipeline): the same launch as the single-shot path, with the chunk's history
struct FirChunkJob {
    FirHandle *h;
    int mode, L, M;
};
static int fir_chunk_kernel(void *self, const void *x_dev, int64_t n_k, int64_t n_hist, void *y_dev, int64_t)
{
    const FirChunkJob *j = static_cast<const FirChunkJob *>(self);
    if (j->mode == 0) return fir_filter_any(j->h, x_dev, n_k, n_hist, y_dev);
    if (j->L == 1) return fir_dn_any(j->h, x_dev, n_k, n_hist, j->M, y_dev);
    return fir_updn_any(j->h, x_dev, n_k, n_hist, j->L, j->M, y_dev);
}
// the job on another slot: same filter, tables on that slot's device (clone made once, owned by the handle)
struct FirChunkJobs {
    FirChunkJob home;                 // the caller's handle
    FirChunkJob other[kMaxSlots];     // its clones, filled as slots ask for them
};
static void *fir_job_on_slot(void *base, int slot)
{
    FirChunkJobs *js = static_cast<FirChunkJobs *>(base);
    FirHandle *h = js->home.h;
    if (slot == h->slot) return &js->home;
    if ((int)h->clones.size() < kMaxSlots) h->clones.resize(kMaxSlots, nullptr);
    if (!h->clones[slot]) {
        h->clones[slot] = fir_derive(h, 0, h->ntaps, slot);
    }
    js->other[slot] = FirChunkJob{static_cast<FirHandle *>(h->clones[slot]), js->home.mode, js->home.L, js->home.M};
    return &js->other[slot];
}

static int fir_host_call(skdsp_handle hh, const void *x, int64_t n, int L, int M, int mode, void *y, int max_slots = 0)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir: not a FIR handle");
    SK_CHECK(n >= 0 && L >= 1 && M >= 1, SKDSP_ERR_BADARG, "fir: bad arguments (n=%lld L=%d M=%d)", (long long)n, L, M);
    const size_t esz = dtype_size(h->dtype);
    const int64_t n_out = mode == 0 ? n : (n * L) / M;
    if (n_out == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "fir: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (opt().host_pipeline && n > (((int64_t)3 << opt().host_chunk_log2) >> 1)) {
        // long vector: chunk pipeline (and every bound slot); exact by construction (n_hist)
        const int64_t hist = L > 1 ? (h->ntaps - 1 + L - 1) / L : h->ntaps - 1;
        const ChunkPlan p = plan_chunks(n, mode == 0 ? 1 : L, mode == 0 ? 1 : M, hist, esz, h->wide_out && !dtype_double(h->dtype),
                                        opt().host_chunk_log2);
        FirChunkJobs jobs;
        jobs.home = FirChunkJob{h, mode, L, M};
        return run_on_slots(p, (const char *)x, (char *)y, fir_chunk_kernel, fir_job_on_slot, &jobs, true, max_slots);
    }
    void *x_dev = nullptr, *y_dev = nullptr;
    int rc = stage_in(x, (size_t)n * esz, &x_dev);
    if (rc) return rc;
    if ((rc = ws_reserve(1, (size_t)n_out * esz + 256, &y_dev))) return rc;
    if (mode == 0) rc = fir_filter_any(h, x_dev, n, 0, y_dev);
    else if (L == 1) rc = fir_dn_any(h, x_dev, n, 0, M, y_dev);
    else rc = fir_updn_any(h, x_dev, n, 0, L, M, y_dev);
    if (rc) return rc;
    return stage_out(y, y_dev, (size_t)n_out * esz, h);
}

// ---- N-D inputs: rows of one launch ---------------------------------------------------------------------------------
// lfilter(b, [1], x) filters along the last axis of an N-D array in one call (multirate_helper.py:108).  A FIR forgets
// after Ntaps-1 samples, so the rows are laid end to end with Ntaps-1 zeros between them and filtered as ONE signal from
// rest: every output sees exactly the window a launch over its row alone would see (zeros in front of every row), so the
// results agree to the kernels' rounding (the overlap-save tile boundaries fall elsewhere).  Host form: one pitched copy in, one launch, one pitched copy out;
// device form: the two pitched copies are device-to-device.  Costs (Ntaps-1)/n extra samples.
constexpr size_t kRowsBlockBudget = (size_t)16 << 30;   // bytes of the staged block of an N-D call (its output block is as large again)
static int64_t fir_rows_pitch(FirHandle *h, int64_t n) { return (int64_t)round_up((size_t)(n + fir_head(h, n)->ntaps - 1), 4); }

static int fir_rows_run(FirHandle *h, int64_t n, int64_t nrow, int64_t pitch, void *xp, void *yp)
{
    h = fir_head(h, n);   // (rows shorter than the filter: only the first n taps are ever reached)
    const size_t esz = dtype_size(h->dtype);
    // zeros between the rows (the last row needs none behind it)
    if (nrow > 1)
        SK_HIP(hipMemset2DAsync((char *)xp + (size_t)n * esz, (size_t)pitch * esz, 0, (size_t)(pitch - n) * esz, (size_t)(nrow - 1), ctx().stream));
    return fir_filter_any(h, xp, (nrow - 1) * pitch + n, 0, yp);
}

int skdsp_fir_filter_rows(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, void *y)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter_rows: not a FIR handle");
    SK_CHECK(n >= 0 && nrow >= 0 && nrow < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "fir_filter_rows: bad arguments");
    if (n == 0 || nrow == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "fir_filter_rows: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = dtype_size(h->dtype);
    const int64_t pitch = fir_rows_pitch(h, n);
    const size_t total = (size_t)nrow * (size_t)pitch * esz;
    // one block holds every row behind its zeros: refused beyond what a pitched copy takes / a sane staging budget (the caller then filters
    // row by row, each through the chunk pipeline)
    SK_CHECK((size_t)pitch * esz * 2 < ((size_t)1 << 31) && total <= kRowsBlockBudget, SKDSP_ERR_UNSUPPORTED,
             "fir_filter_rows: %lld rows of %lld samples do not fit one staged block (%zu bytes)", (long long)nrow, (long long)n, total);
    void *base = nullptr, *yp = nullptr;
    const bool wide = h->wide_out && !dtype_double(h->dtype);
    int rc = ws_reserve(0, kHeadroomBytes + (wide ? 2 : 1) * total + 256, &base);
    if (rc) return rc;
    void *xp = (char *)base + kHeadroomBytes;
    if ((rc = ws_reserve(1, total + 256, &yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(xp, (size_t)pitch * esz, x, (size_t)n * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyHostToDevice, ctx().stream));
    if ((rc = fir_rows_run(h, n, nrow, pitch, xp, yp))) return rc;
    size_t osz = esz;
    if (wide) {   // widen on the device (the staged input is done with in stream order)
        if ((rc = widen_launch(yp, (int64_t)(total / 4), xp, ctx().stream))) return rc;
        yp = xp;
        osz = 2 * esz;
    }
    SK_HIP(hipMemcpy2DAsync(y, (size_t)n * osz, yp, (size_t)pitch * osz, (size_t)n * osz, (size_t)nrow, hipMemcpyDeviceToHost, ctx().stream));
    return sync_checked();
}

int skdsp_fir_filter_rows_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter_rows: not a FIR handle");
    SK_CHECK(n >= 0 && nrow >= 0 && nrow < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "fir_filter_rows: bad arguments");
    if (n == 0 || nrow == 0) return SKDSP_OK;
    SK_CHECK(x_stride >= n && y_stride >= n, SKDSP_ERR_BADARG, "fir_filter_rows: row stride below the row length");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = dtype_size(h->dtype);
    const int64_t pitch = fir_rows_pitch(h, n);
    const size_t total = (size_t)nrow * (size_t)pitch * esz;
    SK_CHECK((size_t)pitch * esz < ((size_t)1 << 31) && (size_t)x_stride * esz < ((size_t)1 << 31) && (size_t)y_stride * esz < ((size_t)1 << 31) &&
                 total <= kRowsBlockBudget, SKDSP_ERR_UNSUPPORTED,
             "fir_filter_rows_dev: %lld rows of %lld samples do not fit one staged block (%zu bytes)", (long long)nrow, (long long)n, total);
    void *base = nullptr, *yp = nullptr;
    int rc = ws_reserve(0, kHeadroomBytes + total + 256, &base);
    if (rc) return rc;
    void *xp = (char *)base + kHeadroomBytes;
    if ((rc = ws_reserve(1, total + 256, &yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(xp, (size_t)pitch * esz, x_dev, (size_t)x_stride * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyDeviceToDevice, ctx().stream));
    if ((rc = fir_rows_run(h, n, nrow, pitch, xp, yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(y_dev, (size_t)y_stride * esz, yp, (size_t)pitch * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyDeviceToDevice, ctx().stream));
    return SKDSP_OK;
}

int skdsp_fir_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return fir_host_call(h, x, n, 1, 1, 0, y); }

int skdsp_fir_filter_sharded(skdsp_handle h, const void *x, int64_t n, void *y, int ngpu)
{
    {
        API_BEGIN;
        SK_CHECK(ngpu >= 0 && ngpu <= slot_count(), SKDSP_ERR_BADARG, "fir_filter_sharded: ngpu = %d, %d slots bound (skdsp_init_devices)", ngpu,
                 slot_count());
    }
    return fir_host_call(h, x, n, 1, 1, 0, y, ngpu);   // (at most ngpu slots; 0: every bound one)
}
int skdsp_fir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return fir_host_call(h, x, n, L, 1, 1, y); }
int skdsp_fir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return fir_host_call(h, x, n, 1, M, 1, y); }
int skdsp_fir_updn(skdsp_handle h, const void *x, int64_t n, int L, int M, void *y) { return fir_host_call(h, x, n, L, M, 1, y); }

}  // extern "C"
