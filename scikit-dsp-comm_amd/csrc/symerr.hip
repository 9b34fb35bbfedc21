// symerr.hip -- the symbol-error tools of the classical BER loops: digitalcom.xcorr (digitalcom.py:1163-1179 of the reference), qam_sep
// (:495-582), qpsk_bep (:723-790) and bpsk_bep (:793-846).  gfx950.  The plans, the index algebra, the quantiser and the per-element decisions
// are symerr_core.hpp, shared with tests/host/symerr_emul.cpp.
//
//   lagcorr_kernel    one workgroup per (group of 256 lags, partition of the 1024-sample tiles): b's tile and a's window (indices mod K) staged
//                     in LDS as re / im planes, each lane 4 lags x 4 samples per step in registers (22 LDS reads for 64 float64 FMAs), the four
//                     waves' sums added in wave order, one partial per (partition, lag) to scratch.  Group 0 also sums |a|^2 and |b|^2.
//   lagmerge_kernel   one thread per lag (and one for the energies): the partitions added in their order.
//   symcount_kernel   work item = (row, 2048 symbols): quantise / rotate / compare per symbol, lanes and waves reduced by shuffles and LDS, four
//                     integer atomics per work item into the row's int64[4].
// No float atomics: two runs give the same bits, integer-valued streams give exact integers.  Nothing outside a call's windows is read.
#include "skdsp_internal.hpp"
#include "symerr_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ double ld_f32(const float *g) const { return (double)*g; }
    __device__ __forceinline__ double ld_f64(const double *g) const { return *g; }
    __device__ __forceinline__ void ld_c64(const float *g, double *re, double *im) const
    {
        const float2 q = *reinterpret_cast<const float2 *>(g);
        *re = (double)q.x;
        *im = (double)q.y;
    }
    __device__ __forceinline__ void ld_c128(const double *g, double *re, double *im) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(g);
        *re = q.x;
        *im = q.y;
    }
    __device__ __forceinline__ void ld_f64x2(const double *g, double *a, double *b) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(g);
        *a = q.x;
        *b = q.y;
    }
    __device__ __forceinline__ void st_f64x2(double *g, double a, double b) const { *reinterpret_cast<double2 *>(g) = make_double2(a, b); }
};

struct DevLds {
    double *w;
    __device__ __forceinline__ double ld(int i) const { return w[i]; }
    __device__ __forceinline__ void st(int i, double v) const { w[i] = v; }
};

// ------------------------------------------------------------------------------------------------------------------ lag correlation
struct LagArgs {
    const void *a, *b;
    double *scratch;
    sye::LagPlan plan;
};

__global__ __launch_bounds__(sye::kThreads) void lagcorr_kernel(LagArgs a)
{
    __shared__ double image[sye::kLdsDoubles];
    const DevLds L = {image};
    const DevMem mem;
    const int t = threadIdx.x;
    const int g = (int)(blockIdx.x % (unsigned)a.plan.ngroups), part = (int)(blockIdx.x / (unsigned)a.plan.ngroups);
    sye::LagAcc acc;
    for (int j = 0; j < sye::kRL; ++j) acc.re[j] = acc.im[j] = 0.0;
    double e1 = 0.0, e2 = 0.0;
    for (int64_t tile = sye::lag_tile_first(a.plan, part); tile < sye::lag_tile_end(a.plan, part); ++tile) {
        __syncthreads();                               // the previous tile has been read
        sye::lag_stage(mem, a.plan, a.a, a.b, tile, g, t, L);
        __syncthreads();
        if (g == 0) sye::lag_energy(a.plan, tile, t, L, &e1, &e2);
        sye::lag_mac(a.plan, g, t, L, acc);
    }
    __syncthreads();
    sye::lag_put(t, L, acc, e1, e2);
    __syncthreads();
    sye::lag_store(mem, a.plan, g, part, t, L, a.scratch);
}

struct MergeArgs {
    const double *scratch;
    double *r, *e;
    sye::LagPlan plan;
};

__global__ __launch_bounds__(sye::kThreads) void lagmerge_kernel(MergeArgs a)
{
    const DevMem mem;
    sye::lag_merge_item(mem, a.plan, a.scratch, (int64_t)blockIdx.x * sye::kThreads + threadIdx.x, a.r, a.e);
}

// ------------------------------------------------------------------------------------------------------------------ the count
struct CntArgs {
    const void *tx, *x;
    unsigned long long *counts;
    uint32_t items;                        // per row
    sye::CntPlan plan;
};

__global__ __launch_bounds__(sye::kThreads) void symcount_kernel(CntArgs a)
{
    __shared__ int32_t wave_sum[sye::kWaves][4];
    const DevMem mem;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const char *tx = static_cast<const char *>(a.tx) + row * a.plan.tx_stride * sye::elem_bytes(a.plan.tx_dtype);
    const char *x = static_cast<const char *>(a.x) + row * a.plan.x_stride * sye::elem_bytes(a.plan.x_dtype);
    sye::Cnt c = {{0, 0, 0, 0}};
    sye::cnt_thread(mem, a.plan, tx, x, it, t, c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int32_t v = c.c[q];
        for (int d = sye::kLane / 2; d > 0; d >>= 1) v += __shfl_down(v, d, sye::kLane);
        if ((t & (sye::kLane - 1)) == 0) wave_sum[t / sye::kLane][q] = v;
    }
    __syncthreads();
    if (t < 4) {
        int64_t s = 0;
        for (int w = 0; w < sye::kWaves; ++w) s += wave_sum[w][t];
        if (s != 0) atomicAdd(a.counts + 4 * row + t, (unsigned long long)s);   // (two's complement: negative sums wrap to the right int64)
    }
}

bool grid_fits(int64_t items, int64_t nrow) { return items == 0 || nrow <= (((int64_t)1 << 31) - 1) / items; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int lagcorr_check(int64_t len, int64_t n_lags, int a_dtype, int b_dtype, int quant_levels, int64_t *n_out, int64_t *first_lag)
{
    sye::LagPlan p;
    const char *why = sye::lag_plan_make(len, n_lags, a_dtype, b_dtype, quant_levels, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "lag_corr: %s", why);
    if (n_out) *n_out = p.nl;
    if (first_lag) *first_lag = p.l0;
    return SKDSP_OK;
}

size_t lagcorr_scratch_bytes(int64_t len, int64_t n_lags)
{
    sye::LagPlan p;
    if (sye::lag_plan_make(len, n_lags, 0, 0, 0, &p)) return 0;
    return (size_t)sye::lag_scratch_doubles(p) * sizeof(double) + 256;
}

// r_dev: nl complex128, e_dev: (E1, E2), scratch_dev: lagcorr_scratch_bytes; all 16-byte aligned
int lagcorr_launch(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, void *scratch_dev, void *r_dev,
                   double *e_dev, hipStream_t s)
{
    LagArgs a;
    const char *why = sye::lag_plan_make(len, n_lags, a_dtype, b_dtype, quant_levels, &a.plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "lag_corr: %s", why);
    if (a.plan.K == 0) return SKDSP_OK;
    SK_CHECK(a_dev && b_dev && scratch_dev && r_dev && e_dev, SKDSP_ERR_BADARG, "lag_corr: null pointer");
    SK_CHECK(((uintptr_t)a_dev & (dtype_size(a_dtype) - 1)) == 0 && ((uintptr_t)b_dev & (dtype_size(b_dtype) - 1)) == 0, SKDSP_ERR_BADARG,
             "lag_corr: the streams must be aligned to their elements");
    SK_CHECK((((uintptr_t)scratch_dev | (uintptr_t)r_dev | (uintptr_t)e_dev) & 15) == 0, SKDSP_ERR_BADARG, "lag_corr: the results must be 16-byte aligned");
    a.a = a_dev;
    a.b = b_dev;
    a.scratch = static_cast<double *>(scratch_dev);
    hipLaunchKernelGGL(lagcorr_kernel, dim3((unsigned)(a.plan.ngroups * a.plan.nparts)), dim3(sye::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    MergeArgs m = {a.scratch, static_cast<double *>(r_dev), e_dev, a.plan};
    hipLaunchKernelGGL(lagmerge_kernel, dim3((unsigned)((a.plan.nl + 1 + sye::kThreads - 1) / sye::kThreads)), dim3(sye::kThreads), 0, s, m);
    SK_HIP(hipGetLastError());
    note_path("lagcorr");
    return SKDSP_OK;
}

int symcount_check(int tx_dtype, int64_t tx_stride, int64_t t0, int x_dtype, int64_t x_stride, int64_t start, int64_t step, int64_t r0, int64_t n, int64_t nrow, int mode,
                   int levels, int kphase)
{
    sye::CntPlan p;
    const char *why = sye::cnt_plan_make(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, mode, levels, kphase, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "sym_count: %s", why);
    SK_CHECK(nrow >= 0 && grid_fits(sye::cnt_items_per_row(n), nrow), SKDSP_ERR_BADARG, "sym_count: %lld rows of %lld symbols in one launch", (long long)nrow, (long long)n);
    return SKDSP_OK;
}

// counts_dev: nrow x int64[4] (sums 0 ... 2, then the elements that break a precondition), zeroed here on the stream
int symcount_launch(const void *tx_dev, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x_dev, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                    int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts_dev, hipStream_t s)
{
    int rc = symcount_check(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase);
    if (rc || nrow == 0) return rc;
    SK_CHECK(counts_dev && ((uintptr_t)counts_dev & 7) == 0, SKDSP_ERR_BADARG, "sym_count: the counts must be an 8-byte aligned pointer");
    SK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)nrow * 4 * sizeof(int64_t), s));
    if (n == 0) return SKDSP_OK;
    SK_CHECK(tx_dev && x_dev, SKDSP_ERR_BADARG, "sym_count: null pointer");
    SK_CHECK(((uintptr_t)tx_dev & (dtype_size(tx_dtype) - 1)) == 0 && ((uintptr_t)x_dev & (dtype_size(x_dtype) - 1)) == 0, SKDSP_ERR_BADARG,
             "sym_count: the streams must be aligned to their elements");
    CntArgs a;
    sye::cnt_plan_make(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, mode, levels, kphase, &a.plan);
    a.tx = tx_dev;
    a.x = x_dev;
    a.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    a.items = (uint32_t)sye::cnt_items_per_row(n);
    hipLaunchKernelGGL(symcount_kernel, dim3((unsigned)(a.items * nrow)), dim3(sye::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("symcount");
    return SKDSP_OK;
}

}  // namespace skdsp
