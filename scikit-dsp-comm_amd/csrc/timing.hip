// timing.hip -- non-data-aided symbol timing recovery over a frame set, synchronization.NDA_symb_sync per row (synchronization.py:43-166 of the
// reference).  gfx950.  The recipe, the plans and the per-thread functions are timing_core.hpp, shared with tests/host/nda_emul.cpp.
//
//   nda_rows_kernel   one wave64 per workgroup, 64 rows, a lane per row.  Per tile of 64 rows x 16 loop iterations (and the Ns + 2 samples around them): the
//                     samples requested one tile ahead sit in registers while the wave walks the current tile out of LDS, symbol-major -- each lane coasts
//                     to its next underflow, the lanes take the heavy step (Ns interpolants, the smoothing sum, atan2) together.  Raw symbols, timing
//                     errors and the rows' counts leave from here.  Specialised on (interpolator order, sample width).
//   nda_norm_kernel   one workgroup per row: np.std over the row's counts[row] elements in two passes with fixed-order sums, then zz (1 / std).
// No atomics, plain vector loads and stores: two runs give the same bits, and those of the host forms.  Nothing outside a call's rows is read, and nothing
// is written behind counts[row] (or cap) elements of a row.
#include "skdsp_internal.hpp"
#include "timing_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ double ld_f64(const double *g) const { return *g; }
    __device__ __forceinline__ uint64_t ld_u64(const void *g) const { return *static_cast<const uint64_t *>(g); }
    __device__ __forceinline__ void ld_c128(const double *g, double *re, double *im) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(g);
        *re = q.x;
        *im = q.y;
    }
    __device__ __forceinline__ void st_f64(double *g, double v) const { *g = v; }
    __device__ __forceinline__ void st_c64(float *g, float re, float im) const { *reinterpret_cast<float2 *>(g) = make_float2(re, im); }
    __device__ __forceinline__ void st_c128(double *g, double re, double im) const { *reinterpret_cast<double2 *>(g) = make_double2(re, im); }
};

struct DevLds {
    double *w;
    __device__ __forceinline__ void ld2(int i, double *a, double *b) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(w + i);
        *a = q.x;
        *b = q.y;
    }
    __device__ __forceinline__ void st2(int i, double a, double b) const { *reinterpret_cast<double2 *>(w + i) = make_double2(a, b); }
};

struct NdaArgs {
    const void *x;
    void *z;
    double *e;
    int64_t *counts;
    const double *gains;
    double k1, k2;
    tim::Plan plan;
    tim::Loop loop;                                    // (its table pointers are set in the kernel)
    double rot_re[tim::kMaxNs], rot_im[tim::kMaxNs];   // the TED rotation constants, copied to LDS by the kernel
};

template <int IORD, bool C64> __global__ __launch_bounds__(tim::kLane) void nda_rows_kernel(NdaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double nda_image[];
    const DevLds L = {nda_image};
    const DevMem mem;
    __shared__ double rre[tim::kMaxNs], rim[tim::kMaxNs];
    const int t = (int)threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < tim::kMaxNs; ++i) {   // (constant indices: scalar loads of the arguments); visible behind the first barrier below
            rre[i] = a.rot_re[i];
            rim[i] = a.rot_im[i];
        }
    }
    tim::Loop lp = a.loop;
    lp.rot_re = rre;
    lp.rot_im = rim;
    const int64_t group = blockIdx.x;
    const tim::Row w = tim::row_of(mem, a.k1, a.k2, a.gains, group * tim::kLane + t, a.plan.nrow);
    tim::State st = tim::state_rest();
    tim::ring_clear(a.plan, t, L);
    car::Sample regs[tim::kMaxW];
    if (a.plan.tiles > 0) tim::tile_fetch<C64>(mem, a.plan, a.x, group, 0, t, regs);
    for (int64_t tile = 0; tile < a.plan.tiles; ++tile) {
        tim::tile_put<C64>(a.plan, t, regs, L);
        __syncthreads();
        if (tile + 1 < a.plan.tiles) tim::tile_fetch<C64>(mem, a.plan, a.x, group, tile + 1, t, regs);   // in flight under the walk
        tim::tile_walk<IORD>(mem, a.plan, lp, w, group, tile, t, st, L, a.z, a.e);
        __syncthreads();
    }
    const int64_t row = group * tim::kLane + t;
    if (row < a.plan.nrow) a.counts[row] = st.mm - 1;
}

struct NormArgs {
    const double *raw;
    void *y;
    const int64_t *counts;
    tim::NormPlan plan;
};

__global__ __launch_bounds__(tim::kNormThreads) void nda_norm_kernel(NormArgs a)
{
    __shared__ __attribute__((aligned(16))) double slots[2 * tim::kNormThreads];
    const DevLds S = {slots};
    const DevMem mem;
    const int t = (int)threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t n = tim::norm_len(mem, a.plan, a.counts, row);
    if (n == 0) return;                                 // (the whole workgroup)
    tim::norm_sums(mem, a.plan, a.raw, row, n, t, S);
    __syncthreads();
    for (int off = tim::kNormThreads / 2; off >= 1; off >>= 1) {
        tim::norm_tree(off, t, S);
        __syncthreads();
    }
    double sr, si;
    S.ld2(0, &sr, &si);
    const double mr = sr / (double)n, mi = si / (double)n;
    __syncthreads();
    tim::norm_dists(mem, a.plan, a.raw, row, n, t, mr, mi, S);
    __syncthreads();
    for (int off = tim::kNormThreads / 2; off >= 1; off >>= 1) {
        tim::norm_tree(off, t, S);
        __syncthreads();
    }
    double q, unused;
    S.ld2(0, &q, &unused);
    const double rcp = 1.0 / sqrt(q / (double)n);
    tim::norm_store(mem, a.plan, a.raw, a.y, row, n, t, rcp);
}

template <class K> int launch_rows(K kern, const NdaArgs &a, hipStream_t s)
{
    const size_t lds = (size_t)a.plan.lds_doubles * sizeof(double);
    if (lds > 48 * 1024) SK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)a.plan.groups), dim3(tim::kLane), lds, s, a);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

bool aligned_to(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int nda_check(int ns, int L, int iord, int dtype, int outputs, int64_t n, int64_t nrow, int64_t start, int64_t x_stride, int64_t y_stride, int64_t cap)
{
    tim::Plan p;
    const char *why = tim::plan_make(ns, L, iord, dtype, 0, outputs, n, nrow, start, x_stride, y_stride, cap, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "nda_rows: %s (Ns = %d, L = %d, I_ord = %d, n = %lld, nrow = %lld, start = %lld, x_stride = %lld, y_stride = %lld, cap = %lld)", why, ns, L, iord,
             (long long)n, (long long)nrow, (long long)start, (long long)x_stride, (long long)y_stride, (long long)cap);
    return SKDSP_OK;
}

size_t nda_scratch_bytes(int dtype, int outputs, int normalize, int64_t nrow, int64_t cap)
{
    return (dtype == SKDSP_C64 && normalize && (outputs & tim::kOutZ)) ? (size_t)nrow * (size_t)cap * 16 : 0;
}

int nda_launch(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2, const double *gains_dev,
               const double *rot_host, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *scratch_dev, void *z_dev, double *e_dev,
               int64_t *counts_dev, int64_t y_stride, hipStream_t s)
{
    int rc = nda_check(ns, L, iord, dtype, outputs, n, nrow, start, x_stride, y_stride, cap);
    if (rc || nrow == 0) return rc;
    const size_t esz = dtype_size(dtype);
    const bool want_z = (outputs & tim::kOutZ) != 0, want_e = (outputs & tim::kOutE) != 0;
    const bool norm = want_z && normalize && cap > 0, via_scratch = norm && dtype == SKDSP_C64;
    SK_CHECK(rot_host, SKDSP_ERR_BADARG, "nda_rows: the rotation constants are missing");
    SK_CHECK(counts_dev && aligned_to(counts_dev, 8), SKDSP_ERR_BADARG, "nda_rows: the counts must be an 8-byte aligned pointer");
    SK_CHECK((n == 0 || (x_dev && aligned_to(x_dev, esz))) && aligned_to(gains_dev, 8), SKDSP_ERR_BADARG, "nda_rows: the input must be a pointer aligned to its element");
    SK_CHECK(cap == 0 || ((!want_z || (z_dev && aligned_to(z_dev, esz))) && (!want_e || (e_dev && aligned_to(e_dev, 8)))), SKDSP_ERR_BADARG,
             "nda_rows: every selected output must be a pointer aligned to its element");
    SK_CHECK(!via_scratch || (scratch_dev && aligned_to(scratch_dev, 16)), SKDSP_ERR_BADARG, "nda_rows: complex64 symbols are normalised out of a float64 workspace");
    if (n > 0 && cap > 0) {
        const uintptr_t x0 = (uintptr_t)x_dev, x1 = x0 + (uintptr_t)((nrow - 1) * x_stride + start + n) * esz;
        const void *outs[2] = {want_z ? z_dev : nullptr, want_e ? e_dev : nullptr};
        for (int i = 0; i < 2; ++i) {
            const uintptr_t y0 = (uintptr_t)outs[i], y1 = y0 + (uintptr_t)((nrow - 1) * y_stride + cap) * (i == 0 ? esz : 8);
            SK_CHECK(!outs[i] || !(x0 < y1 && y0 < x1), SKDSP_ERR_BADARG, "nda_rows: input and output overlap (in place is not supported)");
        }
    }
    NdaArgs a;
    tim::plan_make(ns, L, iord, dtype, dtype == SKDSP_C64 && !via_scratch, outputs, n, nrow, start, x_stride, y_stride, cap, &a.plan);
    if (via_scratch) a.plan.z_stride = cap;          // the walk's zz goes to the workspace (rows cap apart, complex128); e_tau keeps the caller's stride
    a.loop.ns = ns;
    a.loop.len = 2 * L + 1;
    a.loop.inv_ns = inv_ns;
    a.loop.inv_len = inv_len;
    a.loop.k_eps = k_eps;
    for (int i = 0; i < tim::kMaxNs; ++i) {
        a.rot_re[i] = i < ns ? rot_host[i] : 0.0;
        a.rot_im[i] = i < ns ? rot_host[ns + i] : 0.0;
    }
    a.x = x_dev;
    a.z = via_scratch ? scratch_dev : z_dev;
    a.e = e_dev;
    a.counts = counts_dev;
    a.gains = gains_dev;
    a.k1 = k1;
    a.k2 = k2;
#define SK_NDA(C64) (iord == 1 ? launch_rows(nda_rows_kernel<1, C64>, a, s) : iord == 2 ? launch_rows(nda_rows_kernel<2, C64>, a, s) : launch_rows(nda_rows_kernel<3, C64>, a, s))
    rc = a.plan.c64 ? SK_NDA(true) : SK_NDA(false);
#undef SK_NDA
    if (rc) return rc;
    note_path("nda_rows");
    if (!norm) return SKDSP_OK;
    NormArgs b;
    const char *why = tim::norm_plan_make(dtype == SKDSP_C64, nrow, cap, via_scratch ? cap : y_stride, y_stride, &b.plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "nda_rows: %s", why);
    b.raw = static_cast<const double *>(via_scratch ? scratch_dev : z_dev);
    b.y = z_dev;
    b.counts = counts_dev;
    hipLaunchKernelGGL(nda_norm_kernel, dim3((unsigned)nrow), dim3(tim::kNormThreads), 0, s, b);
    SK_HIP(hipGetLastError());
    note_path("nda_norm");
    return SKDSP_OK;
}

}  // namespace skdsp
