// farrow_core.hpp -- the index algebra of the Farrow resampler (digitalcom.farrow_resample), shared by the gfx950
// kernel (farrow.hip) and the host emulation test (tests/host/farrow_emul.cpp).
//
// The reference loops over outputs j in Python (digitalcom.py:224-234):
//     n_old = int(np.floor(j*Ts_new/Ts_old))
//     mu    = (j*Ts_new - n_old*Ts_old)/Ts_old
//     y[j]  = combine(v_m[n_old+1], mu)
// every operation a float64 operation rounded on its own.  Both divisions are reproduced exactly without a divide:
// with r = RN(1/Ts_old) from the host,
//     q0 = a*r;  e = fma(-q0, Ts_old, a);  q = fma(e, r, q0)
// e is the exact remainder a - q0*Ts_old (q0 is within an ulp of a/Ts_old) and, by Markstein's theorem, q = RN(a/Ts_old)
// for positive normal operands: 3 FP64 operations instead of the ~10 of the IEEE division sequence.  The products and
// sums around them must not fuse, hence the pragma (LABNOTES R5.7: __dmul_rn / __dadd_rn do not stop the backend).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SK_FHD __host__ __device__ __forceinline__
#else
#include <cmath>
#define SK_FHD inline
#endif

namespace skdsp {
namespace farrow {

#if defined(__clang__)
#pragma clang fp contract(off)   // (host builds with g++: -ffp-contract=off)
#endif

// RN(a / b) for b > 0 normal, r = RN(1 / b)
SK_FHD double div_rn(double a, double b, double r)
{
    const double q0 = a * r;
    const double e = __builtin_fma(-q0, b, a);
    return __builtin_fma(e, r, q0);
}

struct Index {
    double n_old;   // floor(j Ts_new / Ts_old), an integer in float64
    double mu;      // (j Ts_new - n_old Ts_old) / Ts_old
};

// output j (exactly representable: j < 2^53)
SK_FHD Index index_of(double j, double ts_old, double ts_new, double r)
{
    const double t = j * ts_new;
    Index o;
    o.n_old = __builtin_floor(div_rn(t, ts_old, r));
    const double d = t - o.n_old * ts_old;
    o.mu = div_rn(d, ts_old, r);
    return o;
}

// i_ord = 1 (y = mu v1 + (1 - mu) v0 with v1 = x[n_old], v0 = x[n_old-1]); x0 = x[n_old+1] enters through lfilter's
// zero weight only, so that a non-finite x0 makes the output non-finite as in the reference.  Bit-exact for finite inputs.
SK_FHD double linear(double mu, double x0, double x1, double x2)
{
    const double v1 = 0.0 * x0 + x1;
    const double v0 = (0.0 * x0 + 0.0 * x1) + x2;
    return mu * v1 + (1.0 - mu) * v0;
}
SK_FHD float linear(float mu, float x0, float x1, float x2)
{
    const float v1 = 0.0f * x0 + x1;
    const float v0 = (0.0f * x0 + 0.0f * x1) + x2;
    return mu * v1 + (1.0f - mu) * v0;
}

// The output count: len(np.arange(0, Ts_old*(n-3) + Ts_old, Ts_new)) = max(0, ceil(stop / Ts_new)), without the arange.
// Returns -1 where NumPy's arange would raise (Ts_new == 0, or a length that is not a finite number).
SK_FHD int64_t out_len(int64_t n, double ts_old, double ts_new)
{
    if (ts_new == 0.0) return -1;
    const double stop = ts_old * (double)(n - 3) + ts_old;
    const double len = stop / ts_new;
    if (!(len == len) || len > 9.0e18 || len < -9.0e18) return -1;
    const double c = __builtin_ceil(len);
    return c > 0.0 ? (int64_t)c : 0;
}

}  // namespace farrow
}  // namespace skdsp
