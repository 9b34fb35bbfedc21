// ols4k_tables.hpp -- host-side (float64) tables of the 4096-point tile (ols4k_core.hpp): inter-pass twiddles and the
// pre-permuted, pre-scaled transfer functions of the interpolator's / decimator's phase filters.  Computed in double,
// rounded ONCE to float.  Host only; shared by fir_up4k.hip / fir_dn4k.hip and tests/host/ols4k_emul.cpp.
#pragma once
#include "ols_tables.hpp"
#include "ols4k_core.hpp"

namespace skdsp {
namespace ols4k {

using ols::cd;
using ols::wexp;

// tw[(k1 - 1) * 256 + t] = W_4096^(t k1), k1 = 1..15
inline void make_tw(std::vector<float2> &tw)
{
    tw.resize(kTwUnits);
    for (int k1 = 1; k1 < 16; ++k1)
        for (int t = 0; t < 256; ++t) {
            const cd w = wexp((long long)t * k1, kN);
            tw[(k1 - 1) * 256 + t] = make_float2((float)w.real(), (float)w.imag());
        }
}

// T2[k2 * 16 + c] = W_256^(c k2)
inline void make_T2(std::vector<float2> &T2)
{
    T2.resize(kT2Units);
    for (int k2 = 0; k2 < 16; ++k2)
        for (int c = 0; c < 16; ++c) {
            const cd w = wexp((long long)c * k2, 256);
            T2[k2 * 16 + c] = make_float2((float)w.real(), (float)w.imag());
        }
}

// BY SLOT of the in-place transform: Hp[j * 256 + t] = (H[k(P16(2j))], H[k(P16(2j + 1))]) / N with k(k3) = k1 + 16 k2 + 256 k3,
// t = 16 k1 + k2; appended to `Hp` (2048 float4 = 32 KiB).
// h: `len` complex taps (len <= 4096).
inline void append_Hp(const cd *h, int len, std::vector<float4> &Hp)
{
    std::vector<cd> H(kN, cd(0, 0));
    for (int k = 0; k < len; ++k) H[k] = h[k];
    ols::fft_host(H);
    const double sc = 1.0 / (double)kN;
    const size_t base = Hp.size();
    Hp.resize(base + 8 * 256);
    for (int j = 0; j < 8; ++j)
        for (int t = 0; t < 256; ++t) {
            const int k1 = t >> 4, k2 = t & 15;
            const cd a = H[k1 + 16 * k2 + 256 * P16(2 * j)] * sc, b = H[k1 + 16 * k2 + 256 * P16(2 * j + 1)] * sc;
            Hp[base + j * 256 + t] = make_float4((float)a.real(), (float)a.imag(), (float)b.real(), (float)b.imag());
        }
}

// the phase filters of multirate_FIR.up / .dn on this tile (ols_tables.hpp)
using ols::up_taps_per_phase;
using ols::up_passes;
using ols::tile_overlap;
using ols::dn_taps_per_phase;
inline void make_up_tables(const double *taps, int ntaps, int comp, int L, bool real_pairs, std::vector<float4> &Hp) { ols::make_up_tables(taps, ntaps, comp, L, real_pairs, Hp, append_Hp); }
inline void make_dn_tables(const double *taps, int ntaps, int comp, int M, std::vector<float4> &Hp) { ols::make_dn_tables(taps, ntaps, comp, M, Hp, append_Hp); }

}  // namespace ols4k
}  // namespace skdsp
