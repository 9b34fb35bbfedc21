// tile_walk.hpp -- what the persistent frequency-domain tile engines share around their passes (fir_up4k.hip, fir_up2k.hip,
// fir_dn4k.hip, fir_bank.hip): the walk's first tile, the 4096-point tile's twiddles in LDS, and the small fences that keep
// vector-memory requests and finished results where the kernels put them.  Device only (included by .hip files); the passes
// themselves are ols4k_core.hpp / ols2k_core.hpp, the order of loads, waits and stores is each kernel's own.
#pragma once
#include "ols_core.hpp"

namespace skdsp {
namespace walk {

using ols::cf;

// The first tile of this workgroup: XCD-contiguous runs per round (workgroups are dealt to the 8 XCDs round-robin, so with a grid
// that is a multiple of 8 the workgroups of one XCD walk neighbouring tiles and share their overlap through that XCD's L2).
__device__ __forceinline__ int64_t first_tile()
{
    return (gridDim.x % 8 == 0) ? (int64_t)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8 : (int64_t)blockIdx.x;
}

// The 4096-point tile's twiddles into LDS (ols4k_core.hpp): T2 as it is and transposed, the 15 x 256 pass-1 twiddles.
// The caller's barrier follows.
__device__ __forceinline__ void twiddles_4k(int t, const float2 *T2, const float2 *tw, cf *T2f, cf *T2t, cf *twl)
{
    const cf w = T2[t];
    T2f[t] = w;
    T2t[(t & 15) * 16 + (t >> 4)] = w;
#pragma unroll
    for (int k = 0; k < 15; ++k) twl[k * 256 + t] = tw[k * 256 + t];
}

// volatile 16-byte load: keeps the request at its program position (the scheduler would otherwise sink a prefetch to its first use)
__device__ __forceinline__ float4 vld(const volatile float4 *p)
{
    float4 r;
    r.x = p->x; r.y = p->y; r.z = p->z; r.w = p->w;
    return r;
}
// this thread's 8 float4 of pass q's transfer function (4096-point tile: 2048 float4 per pass)
__device__ __forceinline__ void load_H(const float4 *Hp, int q, int t, float4 *hh)
{
    int tt = t;   // (opaque copy: the addresses are rebuilt where they are used)
    asm volatile("" : "+v"(tt));
    const volatile float4 *hp = reinterpret_cast<const volatile float4 *>(Hp) + (size_t)q * 2048;
#pragma unroll
    for (int k = 0; k < 8; ++k) hh[k] = vld(hp + (unsigned)(k * 256 + tt));
}

// "these are the results, in these registers, now": without it hipcc carries a finished pass in a form of its own (more live registers per
// pass than its results: fir_up2k.hip measured 24 instead of 16 for its eight -- 142 / 236 / 256 + 68 spilled for 4 / 8 / 12 passes per
// thread; with it 122 / 184 / 250 and no spill)
template <int N> __device__ __forceinline__ void pin(cf *v)
{
#pragma unroll
    for (int i = 0; i < N; i += 8)
        asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i + 1].x), "+v"(v[i + 1].y), "+v"(v[i + 2].x), "+v"(v[i + 2].y), "+v"(v[i + 3].x), "+v"(v[i + 3].y),
                     "+v"(v[i + 4].x), "+v"(v[i + 4].y), "+v"(v[i + 5].x), "+v"(v[i + 5].y), "+v"(v[i + 6].x), "+v"(v[i + 6].y), "+v"(v[i + 7].x), "+v"(v[i + 7].y));
}
// "the values must be in their registers HERE": makes hipcc place its wait for a prefetch at this point (vmcnt retires in order, so a
// wait for a load issued BEHIND a store burst is a wait for the stores' acknowledgements: the kernels wait in front of their stores).
// N float4 of a transfer function ...
template <int N> __device__ __forceinline__ void settle(const float4 *hh)
{
#pragma unroll
    for (int k = 0; k < N; k += 4)
        asm volatile("" ::"v"(hh[k].x), "v"(hh[k].y), "v"(hh[k].z), "v"(hh[k].w), "v"(hh[k + 1].x), "v"(hh[k + 1].y), "v"(hh[k + 1].z), "v"(hh[k + 1].w),
                     "v"(hh[k + 2].x), "v"(hh[k + 2].y), "v"(hh[k + 2].z), "v"(hh[k + 2].w), "v"(hh[k + 3].x), "v"(hh[k + 3].y), "v"(hh[k + 3].z), "v"(hh[k + 3].w)
                     : "memory");
}
// ... and the N samples of a tile requested ahead (XR: a float32 signal, the real parts only)
template <bool XR, int N> __device__ __forceinline__ void settle_x(const cf *v)
{
    if constexpr (XR) {
#pragma unroll
        for (int i = 0; i < N; i += 8)
            asm volatile("" ::"v"(v[i].x), "v"(v[i + 1].x), "v"(v[i + 2].x), "v"(v[i + 3].x), "v"(v[i + 4].x), "v"(v[i + 5].x), "v"(v[i + 6].x), "v"(v[i + 7].x) : "memory");
    } else {
#pragma unroll
        for (int i = 0; i < N; i += 8)
            asm volatile("" ::"v"(v[i].x), "v"(v[i].y), "v"(v[i + 1].x), "v"(v[i + 1].y), "v"(v[i + 2].x), "v"(v[i + 2].y), "v"(v[i + 3].x), "v"(v[i + 3].y),
                         "v"(v[i + 4].x), "v"(v[i + 4].y), "v"(v[i + 5].x), "v"(v[i + 5].y), "v"(v[i + 6].x), "v"(v[i + 6].y), "v"(v[i + 7].x), "v"(v[i + 7].y)
                         : "memory");
    }
}

}  // namespace walk
}  // namespace skdsp
