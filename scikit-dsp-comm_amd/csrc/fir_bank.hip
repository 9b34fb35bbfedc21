// fir_bank.hip -- B frequency-shifted copies of ONE FIR over ONE input: the streaming cross-ambiguity function sigsys.fft_caf
// (sigsys.py:2696-2781).  The reference overlap-saves with a 2 F-point FFT and rolls the spectrum of g = conj(h_ref[::-1]) by
// s_j bins per slice; rolling by s_j bins IS the filter g_j[n] = g[n] exp(2 pi i s_j n / (2 F)), and since len(g) <= F the kept half
// of a block holds no circular wrap:  y[j, m] = sum_{n < P} g_j[n] x[m - n], x[< 0] = 0.  All rows read the same x.
//
// One workgroup per (input tile, band group): the 4096-point tile (ols4k_core.hpp: 256 threads x 16 points) is loaded and
// transformed ONCE, its spectrum stays in registers, and every band of the group is one pointwise product with that band's
// pre-permuted transfer function + one inverse transform + V = 4096 - OV contiguous complex64 outputs into row j
// (OV = P - 1 rounded up to 256, at most 2048).  A float32 signal is loaded into the real parts; there is no complex copy of it.
// HBM traffic = the input once per band group (+ OV / V overlap) and every row once; the band tables (32 KiB each, built in
// float64 and rounded once) stream from L2.  Algorithmic bytes: 8 n (1 + B) (complex64), against 16 n B for one launch per band.
//
// Non-finite samples: one inf / nan among a tile's 4096 inputs makes every result of every band non-finite, where the sum above
// confines it to the P outputs per row that multiply it.  A workgroup notes such a tile (careful.hpp: careful_note) and, behind
// its loop, recomputes the outputs it stored for it by the direct sum in float64 over that band's modulated taps.
#include "skdsp_internal.hpp"
#include "ols4k_tables.hpp"
#include "tile_walk.hpp"

namespace skdsp {

using namespace ols4k;
typedef float bank_v2f __attribute__((ext_vector_type(2)));

constexpr int64_t kBankTableCap = (int64_t)256 << 20;   // bytes of band tables one handle may hold (transfer functions + float64 taps)

struct FirBankHandle : HandleBase {
    int ntaps = 0, nbands = 0, ov = 0, V = 0;
    bool xr = false;             // float32 signal
    DevTable<float2> tw, T2;
    DevTable<float4> Hp;         // nbands x 2048 float4
    DevTable<double> g64;        // nbands x ntaps complex128 (interleaved): the bands' taps as the careful path reads them
};

struct BankArgs {
    const void *x;
    cf *y;
    int64_t n, row_stride;
    const float2 *tw, *T2;
    const float4 *Hp;
    const double *g64;
    int ntaps, nbands;
    int ov, V, a0;           // a0 = ov / 256: first stored 256-block of a tile
    int groups, per;         // band groups; bands per group
    int64_t ntiles, items;   // items = ntiles * groups: item = group * ntiles + tile
};

template <bool XR> __device__ __forceinline__ void bank_load_interior(const BankArgs &A, int64_t in0, int t, cf *v)
{
    if (XR) {
        const float *xp = reinterpret_cast<const float *>(A.x) + in0;
#pragma unroll
        for (int a = 0; a < 16; ++a) v[a] = make_float2(xp[(unsigned)(a * 256 + t)], 0.f);
    } else {
        const bank_v2f *xp = reinterpret_cast<const bank_v2f *>(A.x) + in0;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            const bank_v2f r = xp[(unsigned)(a * 256 + t)];
            v[a] = make_float2(r.x, r.y);
        }
    }
}
// (the first and last tiles of a signal only; zero outside [0, n))
template <bool XR> __device__ __forceinline__ void bank_load_edge(const void *x, int64_t in0, int64_t n, int t, cf *v)
{
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        const int64_t g = in0 + 256 * a + t;
        cf val = make_float2(0.f, 0.f);
        if (g >= 0 && g < n) {
            if (XR) val.x = reinterpret_cast<const float *>(x)[g];
            else val = reinterpret_cast<const cf *>(x)[g];
        }
        v[a] = val;
    }
}

__device__ __forceinline__ void bank_load_H(const BankArgs &A, int band, int t, float4 *hh)
{
    const float4 *hp = A.Hp + (size_t)band * 2048;
#pragma unroll
    for (int k = 0; k < 8; ++k) hh[k] = hp[(unsigned)(k * 256 + t)];
}

// outputs out0 + 256 (a - a0) + t, a >= a0, of row `band`
__device__ __forceinline__ void bank_store(const BankArgs &A, int band, int64_t out0, int t, const cf *out)
{
    const int64_t left = A.n - out0;
    const bool whole = left >= A.V;
    const int lim = (int)(left > kN ? kN : left) - t;   // this lane's samples 256 (a - a0) < lim exist
    bank_v2f *yp = reinterpret_cast<bank_v2f *>(A.y + (size_t)band * A.row_stride + out0) + t;
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        if (a < A.a0) continue;
        if (!whole && 256 * (a - A.a0) >= lim) continue;
        __builtin_nontemporal_store(bank_v2f{out[a].x, out[a].y}, yp + 256 * (a - A.a0));
    }
}

// y[band, m] by the direct sum in float64 (IEEE propagation: the P outputs that multiply a non-finite sample come out non-finite)
template <bool XR> __device__ __forceinline__ void bank_careful_point(const BankArgs &A, int band, int64_t m)
{
    CarefulFir c;
    c.taps = A.g64 + (size_t)band * A.ntaps * 2;
    c.ntaps = A.ntaps;
    c.taps_complex = 1;
    double re = 0.0, im = 0.0;
    if (XR) {
        const float *x = reinterpret_cast<const float *>(A.x);
#pragma unroll 1
        for (int k = 0; k < c.ntaps && k <= m; ++k) {
            const double xv = (double)x[m - k];
            re += c.taps[2 * k] * xv;
            im += c.taps[2 * k + 1] * xv;
        }
    } else {
        careful_fir_point<float, true>(reinterpret_cast<const float *>(A.x), 0, c, 1, 1, m, &re, &im);
    }
    A.y[(size_t)band * A.row_stride + m] = make_float2((float)re, (float)im);
}

// Persistent: min(items, 2 workgroups per CU) workgroups walk the (band group, tile) items, item = group * ntiles + tile, so that
// workgroups running side by side hold neighbouring tiles of the same group (they share their overlap and their band tables in L2).
// The next band's table is requested behind the product with the current one -- in front of the current band's stores (vmcnt retires
// in order: a load issued behind a store burst would wait for the stores' acknowledgements) -- and has the inverse transform to arrive.
template <bool XR> __global__ __launch_bounds__(256, 2) void bank4k_kernel(BankArgs A)
{
    __shared__ cf img[kImgUnits];
    __shared__ cf T2f[kT2Units], T2t[kT2Units];
    __shared__ cf twl[kTwUnits];
    __shared__ unsigned long long noted_word;   // poisoned items, by walk step (careful.hpp)
    const int t = threadIdx.x;
    if (t == 0) noted_word = 0;
    walk::twiddles_4k(t, A.T2, A.tw, T2f, T2t, twl);
    __syncthreads();
    int64_t step = 0;
    for (int64_t item = blockIdx.x; item < A.items; item += gridDim.x, ++step) {
        const int group = (int)(item / A.ntiles);
        const int64_t tile = item - (int64_t)group * A.ntiles;
        const int b0 = group * A.per;
        const int b1 = b0 + A.per < A.nbands ? b0 + A.per : A.nbands;
        const int64_t out0 = tile * A.V;
        const int64_t in0 = out0 - A.ov;
        cf Z[16];
        float4 hh[8];
        bank_load_H(A, b0, t, hh);
        if (in0 >= 0 && in0 + kN <= A.n) {
            bank_load_interior<XR>(A, in0, t, Z);
        } else {
            bank_load_edge<XR>(A.x, in0, A.n, t, Z);
        }
        fwd_pass1(t, Z, twl, img);
        __syncthreads();
        fwd_pass2(t, T2f, img);
        fwd_pass3(t, img, Z);
        bool poisoned = false;
        // (the first inverse pass writes the rows this thread's 16-lane group just read: wave-local, no barrier)
#pragma unroll 1
        for (int band = b0; band < b1; ++band) {
            cf P[16];
            mul_H(hh, Z, P);
            if (band + 1 < b1) bank_load_H(A, band + 1, t, hh);
            inv_pass3(t, T2t, img, P);
            inv_pass2(t, img);
            __syncthreads();
            inv_pass1(t, twl, img, P);
            __syncthreads();   // every wave has read the image before the next band (or item) overwrites it
            poisoned = poisoned || not_finite(P[15]);
            bank_store(A, band, out0, t, P);
        }
        if (__builtin_expect(__any(poisoned), 0)) careful_note(&noted_word, step);
    }
    const unsigned long long noted = careful_noted(&noted_word);
    if (__builtin_expect(noted != 0, 0)) {
        // every thread recomputes the outputs IT stored (program order behind its own stores: no further barrier)
        int64_t k = 0;
        for (int64_t item = blockIdx.x; item < A.items; item += gridDim.x, ++k) {
            if (!careful_step_noted(noted, k)) continue;
            const int group = (int)(item / A.ntiles);
            const int64_t out0 = (item - (int64_t)group * A.ntiles) * A.V;
            const int b0 = group * A.per;
            const int b1 = b0 + A.per < A.nbands ? b0 + A.per : A.nbands;
#pragma unroll 1
            for (int band = b0; band < b1; ++band)
#pragma unroll 1
                for (int i = t; i < A.V; i += 256) {
                    if (out0 + i >= A.n) break;
                    bank_careful_point<XR>(A, band, out0 + i);
                }
        }
    }
}

// How the B bands are split into groups.  Every (group, tile) item costs one forward pass and ceil(B / groups) band passes, and `slots`
// workgroups run at a time, so a launch takes about
//   rounds(groups) x (kBankFwdCost + ceil(B / groups)),   rounds = ceil(ntiles x groups / slots)
// band-pass times; the smallest count of groups that minimises this is taken.  kBankFwdCost = 3: the tile's load (not requested ahead),
// the forward transform and the first table's round trip, measured on 2^22 samples / 257 taps (1093 tiles on 512 slots; tools/time_caf.py,
// option fir_bank_per): 9 bands in one group 0.086 ms against 0.0985 in three, 33 bands in three groups of 11 0.257 against 0.288 in one.
// When the tiles alone fill the device and the bands are few that is ONE group holding all bands (the input is read and transformed
// once); a short signal with many bands is split until the items fill the slots; in between, a split pays where it evens out a ragged
// last round (1093 tiles, 33 bands, 512 slots: 7 rounds of 3 + 11 against 3 of 3 + 33).
constexpr int kBankFwdCost = 3;
static int bank_bands_per_group(int64_t ntiles, int nbands, int64_t slots)
{
    int best = nbands;
    int64_t best_cost = INT64_MAX;
    for (int g = 1; g <= nbands; ++g) {
        const int per = (nbands + g - 1) / g;
        const int gg = (nbands + per - 1) / per;   // groups that actually hold bands
        const int64_t rounds = (ntiles * gg + slots - 1) / slots;
        const int64_t cost = rounds * (kBankFwdCost + per);
        if (cost < best_cost) { best_cost = cost; best = per; }
    }
    return best;
}

int fir_bank_create(const void *taps, int ntaps, int taps_complex, const int64_t *shifts, int nbands, int period, int dtype, HandleBase **out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "fir_bank_create: null out");
    SK_CHECK(taps && ntaps >= 1, SKDSP_ERR_BADARG, "fir_bank_create: need at least one tap");
    SK_CHECK(ntaps - 1 <= 2048, SKDSP_ERR_BADARG, "fir_bank_create: at most 2049 taps (got %d)", ntaps);
    SK_CHECK(shifts && nbands >= 1, SKDSP_ERR_BADARG, "fir_bank_create: need at least one band (got %d)", nbands);
    SK_CHECK(period >= 1, SKDSP_ERR_BADARG, "fir_bank_create: period must be >= 1 (got %d)", period);
    SK_CHECK(dtype == SKDSP_F32 || dtype == SKDSP_C64, SKDSP_ERR_BADARG, "fir_bank_create: the signal must be float32 or complex64 (dtype %d)", dtype);
    const int64_t table_bytes = (int64_t)nbands * (2048 * (int64_t)sizeof(float4) + (int64_t)ntaps * 16);
    SK_CHECK(table_bytes <= kBankTableCap, SKDSP_ERR_BADARG, "fir_bank_create: %d bands of %d taps need %lld bytes of tables (cap %lld)", nbands, ntaps,
             (long long)table_bytes, (long long)kBankTableCap);
    {
        int rc = ensure_init();
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> ctxlk(ctx().mu);
    std::unique_ptr<FirBankHandle> h(new FirBankHandle());
    h->kind = H_FIRBANK;
    h->dtype = dtype;
    h->xr = dtype == SKDSP_F32;
    h->ntaps = ntaps;
    h->nbands = nbands;
    h->ov = ((ntaps - 1 + 255) / 256) * 256;
    h->V = kN - h->ov;
    // band j: g_j[n] = taps[n] exp(2 pi i ((shifts[j] n) mod period) / period): the phase is reduced in integers, float64 throughout
    const double *tp = static_cast<const double *>(taps);
    std::vector<cd> g((size_t)nbands * ntaps);
    std::vector<float4> Hp;
    Hp.reserve((size_t)nbands * 2048);
    for (int j = 0; j < nbands; ++j) {
        const long long s = ((shifts[j] % period) + period) % period;
        cd *gj = g.data() + (size_t)j * ntaps;
        for (int k = 0; k < ntaps; ++k) {
            const cd tap = taps_complex ? cd(tp[2 * k], tp[2 * k + 1]) : cd(tp[k], 0.0);
            gj[k] = tap * std::conj(wexp((s * k) % period, period));
        }
        append_Hp(gj, ntaps, Hp);
    }
    std::vector<float2> tw, T2;
    make_tw(tw);
    make_T2(T2);
    int rc = h->tw.upload(tw);
    if (!rc) rc = h->T2.upload(T2);
    if (!rc) rc = h->Hp.upload(Hp);
    if (!rc) rc = h->g64.upload(reinterpret_cast<const double *>(g.data()), 2 * g.size());
    if (rc) return rc;
    *out = h.release();
    return SKDSP_OK;
}

int fir_bank_launch(HandleBase *hb, const void *x, int64_t n, void *y, int64_t row_stride, hipStream_t s)
{
    note_path("fir_bank4k");
    FirBankHandle *h = static_cast<FirBankHandle *>(hb);
    if (n <= 0) return SKDSP_OK;
    SK_CHECK(row_stride >= n, SKDSP_ERR_BADARG, "fir_bank: row_stride %lld < n %lld", (long long)row_stride, (long long)n);
    SK_CHECK((((uintptr_t)x) & (h->xr ? 3 : 7)) == 0 && (((uintptr_t)y) & 7) == 0, SKDSP_ERR_BADARG, "fir_bank: x / y not element-aligned");
    BankArgs A;
    A.x = x; A.y = static_cast<cf *>(y); A.n = n; A.row_stride = row_stride;
    A.tw = h->tw.dev; A.T2 = h->T2.dev; A.Hp = h->Hp.dev; A.g64 = h->g64.dev;
    A.ntaps = h->ntaps; A.nbands = h->nbands;
    A.ov = h->ov; A.V = h->V; A.a0 = h->ov / 256;
    A.ntiles = (n + h->V - 1) / h->V;
    const int64_t slots = 2 * (int64_t)ctx().num_cus;
    A.per = bank_bands_per_group(A.ntiles, h->nbands, slots);
    if (opt().fir_bank_per > 0) A.per = opt().fir_bank_per < h->nbands ? opt().fir_bank_per : h->nbands;
    A.groups = (h->nbands + A.per - 1) / A.per;
    A.items = A.ntiles * A.groups;
    SK_CHECK(A.items < (int64_t)1 << 31, SKDSP_ERR_BADARG, "fir_bank: too many tiles");
    const int64_t grid = A.items < slots ? A.items : slots;
    if (h->xr) hipLaunchKernelGGL((bank4k_kernel<true>), dim3((unsigned)grid), dim3(256), 0, s, A);
    else hipLaunchKernelGGL((bank4k_kernel<false>), dim3((unsigned)grid), dim3(256), 0, s, A);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

}  // namespace skdsp
