// farrow.hip -- arbitrary-ratio Farrow resampler, digitalcom.farrow_resample (digitalcom.py:53-235).  gfx950.
//
// Output j of the whole resampled signal is a 4-tap FIR of x around k = n_old + 1 whose taps are polynomials in the
// fractional delay mu (farrow_core.hpp: n_old and mu, exactly as the reference rounds them):
//   i_ord 3: y = ((v3 mu + v2) mu + v1) mu + v0      i_ord 2: y = (v2 + v1) mu + v0      i_ord 1: y = mu v1 + (1 - mu) v0
// with v_m[k] = lfilter(w_m, 1, x)[k] over x[k-3 .. k] (x[i] = 0 for i < 0).
//
// One workgroup owns a contiguous run of B = 256 P rows outputs; since n_old never decreases with j its input span is
// [n_old(first) - 2, n_old(last) + 1], which is staged in LDS with 16-byte loads (one sample of margin on either side).
// Every thread then evaluates P consecutive outputs per row from LDS and stores them as one 16-byte nontemporal store.
// A span larger than the LDS array (a down-ratio steeper than 4 - 8 : 1, by sample size) reads its taps straight from global memory.
//
// n_old and mu are always float64.  The weights and the sum run in float64 for float64 / complex128 inputs and, on
// request (flag SKDSP_FARROW_F64), for float32 / complex64 ones; otherwise in float32.  i_ord = 1 in float64 is
// bit-exact against the reference for finite inputs; every tap of the window is multiplied in, so a non-finite sample
// makes exactly the outputs whose window holds it non-finite.
#include "skdsp_internal.hpp"
#include "farrow_core.hpp"

namespace skdsp {
namespace {

constexpr int kThreads = 256;
constexpr int kLdsBytes = 16384;

struct FarrowArgs {
    double ts_old, ts_new, r, alpha;
    int64_t n, n0, count;
    int rows;
};

template <typename SC, int ORD>
__device__ __forceinline__ SC combine(SC mu, SC x0, SC x1, SC x2, SC x3, SC alpha)
{
    // x0 = x[k], x1 = x[k-1], x2 = x[k-2], x3 = x[k-3]
    if constexpr (ORD == 3) {
        const SC c6 = SC(1) / SC(6), c3 = SC(1) / SC(3), h = SC(0.5);
        const SC v3 = (x0 - x3) * c6 + (x2 - x1) * h;
        const SC v2 = (x1 + x3) * h - x2;
        const SC v1 = x1 - x0 * c6 - x2 * h - x3 * c3;
        return ((v3 * mu + v2) * mu + v1) * mu + x2;
    } else if constexpr (ORD == 2) {
        const SC v2 = alpha * ((x0 - x1) - (x2 - x3));
        const SC v1 = (SC(1) + alpha) * x1 + (alpha - SC(1)) * x2 - alpha * (x0 + x3);
        return (v2 + v1) * mu + x2;
    } else {
        (void)x3; (void)alpha;
        return farrow::linear(mu, x0, x1, x2);
    }
}

// Taps from the LDS span (STAGED) or straight from global memory (x[i] = 0 outside [0, n)).
template <typename SI, int NC, bool STAGED> struct Taps {
    const SI *src;   // LDS span or x
    int64_t s0, n;
    __device__ __forceinline__ SI get(int64_t i, int c) const
    {
        if constexpr (STAGED) return src[(int)(i - s0) * NC + c];
        else return (i >= 0 && i < n) ? src[i * NC + c] : SI(0);
    }
};

template <typename SI, typename SC, typename SO, int NC, int ORD, bool STAGED>
__device__ __forceinline__ void farrow_rows(const Taps<SI, NC, STAGED> &tp, const FarrowArgs &a, int64_t jb, int64_t je,
                                            SO *__restrict__ y, bool y16)
{
    constexpr int P = 16 / (int)(sizeof(SO) * NC);
    const double jbd = (double)jb;
    const SC alpha = (SC)a.alpha;
    for (int r = 0; r < a.rows; ++r) {
        const int off = (r * kThreads + (int)threadIdx.x) * P;   // < B
        const int64_t j0 = jb + off;
        if (j0 >= je) break;
        SO out[P * NC];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const farrow::Index ix = farrow::index_of(jbd + (double)(off + p), a.ts_old, a.ts_new, a.r);
            const int64_t k = (int64_t)ix.n_old + 1;
            const SC mu = (SC)ix.mu;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const SC x0 = (SC)tp.get(k, c), x1 = (SC)tp.get(k - 1, c), x2 = (SC)tp.get(k - 2, c), x3 = (SC)tp.get(k - 3, c);
                out[p * NC + c] = (SO)combine<SC, ORD>(mu, x0, x1, x2, x3, alpha);
            }
        }
        SO *dst = y + (j0 - a.n0) * NC;
        if (y16 && j0 + P <= je) {
            typedef float nt4_t __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(*reinterpret_cast<const nt4_t *>(out), reinterpret_cast<nt4_t *>(dst));
        } else {
            for (int p = 0; p < P && j0 + p < je; ++p)
#pragma unroll
                for (int c = 0; c < NC; ++c) dst[p * NC + c] = out[p * NC + c];
        }
    }
}

template <typename SI, typename SC, typename SO, int NC, int ORD>
__global__ __launch_bounds__(kThreads) void farrow_kernel(const SI *__restrict__ x, FarrowArgs a, SO *__restrict__ y)
{
    constexpr int P = 16 / (int)(sizeof(SO) * NC);
    constexpr int VE = 16 / (int)(sizeof(SI) * NC);            // input samples per 16-byte load
    constexpr int SMAX = kLdsBytes / (int)(sizeof(SI) * NC);   // samples the LDS span holds
    __shared__ __attribute__((aligned(16))) SI lds[SMAX * NC];

    const int64_t B = (int64_t)kThreads * P * a.rows;
    const int64_t jb = a.n0 + (int64_t)blockIdx.x * B;
    const int64_t je = min(jb + B, a.n0 + a.count);
    const bool y16 = ((uintptr_t)y & 15) == 0;

    // the span: windows x[n_old-2 .. n_old+1] of the first and the last output, plus one sample of margin each side
    const int64_t kf = (int64_t)farrow::index_of((double)jb, a.ts_old, a.ts_new, a.r).n_old;
    const int64_t kl = (int64_t)farrow::index_of((double)(je - 1), a.ts_old, a.ts_new, a.r).n_old;
    int64_t s0 = kf - 3, s1 = kl + 3;
    s0 -= ((s0 % VE) + VE) % VE;
    s1 += (VE - ((s1 % VE) + VE) % VE) % VE;

    if (s1 - s0 > SMAX) {   // (block-uniform) a steep down-ratio: the taps come from global memory
        farrow_rows<SI, SC, SO, NC, ORD, false>(Taps<SI, NC, false>{x, 0, a.n}, a, jb, je, y, y16);
        return;
    }
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const bool x16 = ((uintptr_t)x & 15) == 0;
    const int nv = (int)((s1 - s0) / VE);
    for (int v = threadIdx.x; v < nv; v += kThreads) {
        const int64_t i0 = s0 + (int64_t)v * VE;
        SI *d = lds + v * VE * NC;
        if (x16 && i0 >= 0 && i0 + VE <= a.n) {
            *reinterpret_cast<v4u *>(d) = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(x + i0 * NC));
        } else {
#pragma unroll
            for (int e = 0; e < VE; ++e)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int64_t i = i0 + e;
                    d[e * NC + c] = (i >= 0 && i < a.n) ? x[i * NC + c] : SI(0);
                }
        }
    }
    __syncthreads();
    farrow_rows<SI, SC, SO, NC, ORD, true>(Taps<SI, NC, true>{lds, s0, a.n}, a, jb, je, y, y16);
}

template <typename SI, typename SC, typename SO, int NC>
static void launch_ord(int i_ord, dim3 grid, const void *x, const FarrowArgs &a, void *y, hipStream_t s)
{
    if (i_ord == 3)
        hipLaunchKernelGGL((farrow_kernel<SI, SC, SO, NC, 3>), grid, dim3(kThreads), 0, s, (const SI *)x, a, (SO *)y);
    else if (i_ord == 2)
        hipLaunchKernelGGL((farrow_kernel<SI, SC, SO, NC, 2>), grid, dim3(kThreads), 0, s, (const SI *)x, a, (SO *)y);
    else
        hipLaunchKernelGGL((farrow_kernel<SI, SC, SO, NC, 1>), grid, dim3(kThreads), 0, s, (const SI *)x, a, (SO *)y);
}

}  // namespace

int farrow_len(int64_t n, double ts_old, double ts_new, int64_t *n_out)
{
    SK_CHECK(n_out && n >= 0, SKDSP_ERR_BADARG, "farrow: bad arguments");
    const int64_t len = farrow::out_len(n, ts_old, ts_new);
    SK_CHECK(len >= 0, SKDSP_ERR_BADARG, "farrow: no output length for Ts_old=%g Ts_new=%g", ts_old, ts_new);
    *n_out = len;
    return SKDSP_OK;
}

int farrow_launch(const void *x, int64_t n, int dtype, double ts_old, double ts_new, int i_ord, double alpha, int64_t n0,
                  int64_t count, int flags, void *y, hipStream_t s)
{
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "farrow: bad dtype %d", dtype);
    SK_CHECK(i_ord >= 1 && i_ord <= 3, SKDSP_ERR_BADARG, "farrow: i_ord must be 1, 2 or 3 (got %d)", i_ord);
    int64_t N = 0;
    int rc = farrow_len(n, ts_old, ts_new, &N);
    if (rc) return rc;
    SK_CHECK(n0 >= 0 && count >= 0 && n0 + count <= N, SKDSP_ERR_BADARG,
             "farrow: outputs [%lld, %lld) outside the %lld of the signal", (long long)n0, (long long)(n0 + count), (long long)N);
    if (count == 0) return SKDSP_OK;
    if (ts_old < 0 && ts_new < 0) {   // (only a pair of negative periods has outputs: the same ones as the positive pair)
        ts_old = -ts_old;
        ts_new = -ts_new;
    }
    const double r = 1.0 / ts_old;
    SK_CHECK(ts_old >= 2.2250738585072014e-308 && ts_new > 0 && r < 1.7976931348623157e308 && ts_new < 1.7976931348623157e308,
             SKDSP_ERR_BADARG, "farrow: periods Ts_old=%g Ts_new=%g outside the normal range", ts_old, ts_new);
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "farrow: null pointer");

    const bool narrow = !dtype_double(dtype), cplx = dtype == SKDSP_C64 || dtype == SKDSP_C128;
    const bool wide = narrow && (flags & SKDSP_FARROW_WIDE), f64 = !narrow || (flags & SKDSP_FARROW_F64);
    const int out_bytes = (narrow && !wide ? 4 : 8) * (cplx ? 2 : 1);
    const int in_bytes = (int)dtype_size(dtype);
    const int P = 16 / out_bytes;
    // outputs per workgroup: up to 2048, fewer where the span of a steeper down-ratio would overflow the LDS array
    const double in_per_out = ts_new / ts_old;
    const int smax = kLdsBytes / in_bytes;
    int rows = 2048 / (kThreads * P);
    while (rows > 1 && (double)kThreads * P * rows * in_per_out + 16 > smax) rows /= 2;
    FarrowArgs a{ts_old, ts_new, r, alpha, n, n0, count, rows};
    const int64_t B = (int64_t)kThreads * P * rows;
    const int64_t blocks = (count + B - 1) / B;
    SK_CHECK(blocks < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "farrow: %lld outputs in one launch", (long long)count);
    const dim3 grid((unsigned)blocks);

    switch (dtype) {
    case SKDSP_F32:
        if (f64) { if (wide) launch_ord<float, double, double, 1>(i_ord, grid, x, a, y, s); else launch_ord<float, double, float, 1>(i_ord, grid, x, a, y, s); }
        else     { if (wide) launch_ord<float, float, double, 1>(i_ord, grid, x, a, y, s);  else launch_ord<float, float, float, 1>(i_ord, grid, x, a, y, s); }
        break;
    case SKDSP_C64:
        if (f64) { if (wide) launch_ord<float, double, double, 2>(i_ord, grid, x, a, y, s); else launch_ord<float, double, float, 2>(i_ord, grid, x, a, y, s); }
        else     { if (wide) launch_ord<float, float, double, 2>(i_ord, grid, x, a, y, s);  else launch_ord<float, float, float, 2>(i_ord, grid, x, a, y, s); }
        break;
    case SKDSP_F64: launch_ord<double, double, double, 1>(i_ord, grid, x, a, y, s); break;
    default:        launch_ord<double, double, double, 2>(i_ord, grid, x, a, y, s); break;
    }
    SK_HIP(hipGetLastError());
    note_path("farrow");
    return SKDSP_OK;
}

}  // namespace skdsp
