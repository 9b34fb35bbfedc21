// carrier.hip -- decision-directed carrier phase tracking over a frame set, synchronization.DD_carrier_sync per row (synchronization.py:169-275 of the
// reference), and the impairment helpers phase_step / time_step over rows (:278-313).  gfx950.  The step, the plans and the per-thread functions are
// carrier_core.hpp, shared with tests/host/carrier_emul.cpp.
//
//   carrier_rows_kernel   one wave64 per workgroup, 64 rows, a lane per row.  Per tile of 64 rows x 8 symbols: the samples requested one tile ahead
//                         sit in registers while the wave walks the current tile out of LDS, so the loads' latency lies under the serial chain;
//                         the selected outputs go back through LDS and leave as runs along the rows.  Specialised on (family, detector type, sample width).
//   impair_rows_kernel    one thread per output element: time_step's gather with zero fill, phase_step's pick of every ns-th sample and rotation.
// No atomics, plain vector loads and stores: two runs give the same bits, and those of the host forms.  Nothing outside a call's rows is read or written.
#include "skdsp_internal.hpp"
#include "carrier_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ double ld_f64(const double *g) const { return *g; }
    __device__ __forceinline__ uint64_t ld_u64(const void *g) const { return *static_cast<const uint64_t *>(g); }
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
    __device__ __forceinline__ void st_f64(double *g, double v) const { *g = v; }
    __device__ __forceinline__ void st_c64(float *g, float re, float im) const { *reinterpret_cast<float2 *>(g) = make_float2(re, im); }
    __device__ __forceinline__ void st_c128(double *g, double re, double im) const { *reinterpret_cast<double2 *>(g) = make_double2(re, im); }
};

struct DevLds {
    double *w;
    __device__ __forceinline__ double ld(int i) const { return w[i]; }
    __device__ __forceinline__ void st(int i, double v) const { w[i] = v; }
    __device__ __forceinline__ void ld2(int i, double *a, double *b) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(w + i);
        *a = q.x;
        *b = q.y;
    }
    __device__ __forceinline__ void st2(int i, double a, double b) const { *reinterpret_cast<double2 *>(w + i) = make_double2(a, b); }
};

struct CarArgs {
    const void *x;
    void *z, *a;
    double *e, *t;
    const double *gains, *r;
    double k1, k2;
    car::Plan plan;
    car::Loop loop;                                  // (its table pointers are set in the kernel)
    double tab_re[sym::kTab], tab_im[sym::kTab];     // MPSK above 4: the decision points, copied to LDS by the kernel
};

template <int FAM, int TYPE, bool C64> __global__ __launch_bounds__(car::kLane) void carrier_rows_kernel(CarArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double carrier_image[];
    const DevLds L = {carrier_image};
    const DevMem mem;
    __shared__ double tre[sym::kTab], tim[sym::kTab];
    const int t = (int)threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < sym::kTab; ++i) {   // (constant indices: scalar loads of the arguments); visible behind the first barrier below
            tre[i] = a.tab_re[i];
            tim[i] = a.tab_im[i];
        }
    }
    car::Loop lp = a.loop;
    lp.tab_re = tre;
    lp.tab_im = tim;
    const int64_t group = blockIdx.x;
    const car::Row w = car::row_of(mem, a.k1, a.k2, a.gains, a.r, group * car::kLane + t, a.plan.nrow);
    car::State st = {0.0, 0.0};
    car::Sample regs[car::kPer];
    car::tile_fetch<C64>(mem, a.plan, a.x, group, 0, t, regs);
    for (int64_t tile = 0; tile < a.plan.tiles; ++tile) {
        car::tile_put<C64>(a.plan, t, regs, L);
        __syncthreads();
        if (tile + 1 < a.plan.tiles) car::tile_fetch<C64>(mem, a.plan, a.x, group, tile + 1, t, regs);   // in flight under the walk
        car::tile_walk<FAM, TYPE>(a.plan, lp, w, group, tile, t, st, L);
        __syncthreads();
        car::tile_store<C64>(mem, a.plan, a.z, a.a, a.e, a.t, group, tile, t, L);
        __syncthreads();
    }
}

struct ImpArgs {
    const void *x;
    void *y;
    const int64_t *shifts;
    const double *factors;
    int64_t shift;
    double c, d;
    uint32_t chunks;      // blocks per row
    car::ImpPlan plan;
};
constexpr int kImpThreads = 256;

__global__ __launch_bounds__(kImpThreads) void impair_rows_kernel(ImpArgs a)
{
    const int64_t row = blockIdx.x / a.chunks, j = (int64_t)(blockIdx.x - row * a.chunks) * kImpThreads + threadIdx.x;
    if (j >= a.plan.n_out) return;
    const int64_t shift = a.shifts ? a.shifts[row] : a.shift;
    const double c = a.factors ? a.factors[2 * row] : a.c, d = a.factors ? a.factors[2 * row + 1] : a.d;
    car::imp_item(DevMem(), a.plan, a.x, a.y, row, j, shift, c, d);
}

template <class K> int launch_rows(K kern, const CarArgs &a, hipStream_t s)
{
    const size_t lds = (size_t)a.plan.lds_doubles * sizeof(double);
    if (lds > 48 * 1024) SK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)a.plan.groups), dim3(car::kLane), lds, s, a);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

bool aligned_to(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int carrier_check(int family, int mod, int type, int dtype, int outputs, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride)
{
    car::Plan p;
    const char *why = car::plan_make(family, mod, type, dtype, outputs, n, nrow, start, step, x_stride, y_stride, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "carrier_rows: %s (M = %d, type = %d, n = %lld, nrow = %lld, start = %lld, step = %lld, x_stride = %lld, y_stride = %lld)", why, mod, type,
             (long long)n, (long long)nrow, (long long)start, (long long)step, (long long)x_stride, (long long)y_stride);
    return SKDSP_OK;
}

int carrier_launch(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop,
                   double k1, double k2, const double *gains_dev, const double *r_dev, double inv_sqrt2, const double *tab_re_host, const double *tab_im_host, int outputs,
                   void *z_dev, void *a_dev, double *e_dev, double *t_dev, int64_t y_stride, hipStream_t s)
{
    int rc = carrier_check(family, mod, type, dtype, outputs, n, nrow, start, step, x_stride, y_stride);
    if (rc || n == 0 || nrow == 0) return rc;
    CarArgs a;
    car::plan_make(family, mod, type, dtype, outputs, n, nrow, start, step, x_stride, y_stride, &a.plan);
    SK_CHECK(family != sym::kMpsk || mod <= 4 || (tab_re_host && tab_im_host), SKDSP_ERR_BADARG, "carrier_rows: MPSK above 4 needs the table of decision points");
    SK_CHECK(family != sym::kQam || r_dev, SKDSP_ERR_BADARG, "carrier_rows: MQAM needs the rows' scales");
    const size_t esz = dtype_size(dtype);
    SK_CHECK(x_dev && aligned_to(x_dev, esz), SKDSP_ERR_BADARG, "carrier_rows: the input must be a pointer aligned to its element");
    SK_CHECK((!(outputs & car::kOutZ) || (z_dev && aligned_to(z_dev, esz))) && (!(outputs & car::kOutA) || (a_dev && aligned_to(a_dev, esz))) &&
                 (!(outputs & car::kOutE) || (e_dev && aligned_to(e_dev, 8))) && (!(outputs & car::kOutT) || (t_dev && aligned_to(t_dev, 8))),
             SKDSP_ERR_BADARG, "carrier_rows: every selected output must be a pointer aligned to its element");
    SK_CHECK(aligned_to(gains_dev, 8) && aligned_to(r_dev, 8), SKDSP_ERR_BADARG, "carrier_rows: the gains and the scales must be 8-byte aligned");
    const uintptr_t x0 = (uintptr_t)x_dev, x1 = x0 + (uintptr_t)((nrow - 1) * x_stride + start + (n - 1) * step + 1) * esz;
    const void *outs[4] = {(outputs & car::kOutZ) ? z_dev : nullptr, (outputs & car::kOutA) ? a_dev : nullptr, (outputs & car::kOutE) ? e_dev : nullptr,
                           (outputs & car::kOutT) ? t_dev : nullptr};
    for (int i = 0; i < 4; ++i) {
        const uintptr_t y0 = (uintptr_t)outs[i], y1 = y0 + (uintptr_t)((nrow - 1) * y_stride + n) * (i < 2 ? esz : 8);
        SK_CHECK(!outs[i] || !(x0 < y1 && y0 < x1), SKDSP_ERR_BADARG, "carrier_rows: input and output overlap (in place is not supported)");
    }
    car::loop_make(family, mod, open_loop, inv_sqrt2, nullptr, nullptr, &a.loop);
    for (int i = 0; i < sym::kTab; ++i) {
        const bool have = family == sym::kMpsk && mod > 4 && i < mod;
        a.tab_re[i] = have ? tab_re_host[i] : 0.0;
        a.tab_im[i] = have ? tab_im_host[i] : 0.0;
    }
    a.x = x_dev;
    a.z = z_dev;
    a.a = a_dev;
    a.e = e_dev;
    a.t = t_dev;
    a.gains = gains_dev;
    a.r = family == sym::kQam ? r_dev : nullptr;
    a.k1 = k1;
    a.k2 = k2;
#define SK_CAR(FAM, C64) (type == 0 ? launch_rows(carrier_rows_kernel<FAM, 0, C64>, a, s) : type == 1 ? launch_rows(carrier_rows_kernel<FAM, 1, C64>, a, s) : launch_rows(carrier_rows_kernel<FAM, 2, C64>, a, s))
    if (a.plan.c64)
        rc = family == sym::kQam ? SK_CAR(sym::kQam, true) : SK_CAR(sym::kMpsk, true);
    else
        rc = family == sym::kQam ? SK_CAR(sym::kQam, false) : SK_CAR(sym::kMpsk, false);
#undef SK_CAR
    if (rc) return rc;
    note_path("carrier_rows");
    return SKDSP_OK;
}

int impair_check(int mode, int dtype, int64_t n, int64_t n_out, int64_t nrow, int64_t ns, int64_t n_step, int64_t x_stride, int64_t y_stride)
{
    car::ImpPlan p;
    const char *why = car::imp_plan_make(mode, dtype, n, n_out, nrow, ns, n_step, x_stride, y_stride, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "%s: %s (n = %lld, n_out = %lld, nrow = %lld, ns = %lld, n_step = %lld, x_stride = %lld, y_stride = %lld)", mode ? "phase_step" : "time_step",
             why, (long long)n, (long long)n_out, (long long)nrow, (long long)ns, (long long)n_step, (long long)x_stride, (long long)y_stride);
    const int64_t chunks = (n_out + kImpThreads - 1) / kImpThreads;
    SK_CHECK(chunks == 0 || nrow <= (((int64_t)1 << 31) - 1) / chunks, SKDSP_ERR_BADARG, "%s: too many (row, chunk) pairs for one launch", mode ? "phase_step" : "time_step");
    return SKDSP_OK;
}

int impair_launch(int mode, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, int64_t shift, const int64_t *shifts_dev,
                  double c, double d, const double *factors_dev, void *y_dev, int64_t n_out, int64_t y_stride, hipStream_t s)
{
    int rc = impair_check(mode, dtype, n, n_out, nrow, ns, n_step, x_stride, y_stride);
    if (rc || n_out == 0 || nrow == 0) return rc;
    const char *name = mode ? "phase_step" : "time_step";
    const size_t esz = dtype_size(dtype);
    SK_CHECK(mode != 0 || shifts_dev || (shift >= 0 && shift < car::kMaxLen), SKDSP_ERR_BADARG, "%s: need 0 <= t_step < 2^40", name);
    SK_CHECK(y_dev && (x_dev || n == 0) && aligned_to(x_dev, esz) && aligned_to(y_dev, esz), SKDSP_ERR_BADARG, "%s: the rows must be pointers aligned to their elements", name);
    SK_CHECK(aligned_to(shifts_dev, 8) && aligned_to(factors_dev, 8), SKDSP_ERR_BADARG, "%s: the per-row values must be 8-byte aligned", name);
    const uintptr_t x0 = (uintptr_t)x_dev, x1 = x0 + (uintptr_t)((nrow - 1) * x_stride + n) * esz, y0 = (uintptr_t)y_dev, y1 = y0 + (uintptr_t)((nrow - 1) * y_stride + n_out) * esz;
    SK_CHECK(!(x0 < y1 && y0 < x1), SKDSP_ERR_BADARG, "%s: input and output overlap (in place is not supported)", name);
    ImpArgs a;
    car::imp_plan_make(mode, dtype, n, n_out, nrow, ns, n_step, x_stride, y_stride, &a.plan);
    a.x = x_dev;
    a.y = y_dev;
    a.shifts = mode == 0 ? shifts_dev : nullptr;
    a.factors = mode == 1 ? factors_dev : nullptr;
    a.shift = shift;
    a.c = c;
    a.d = d;
    a.chunks = (uint32_t)((n_out + kImpThreads - 1) / kImpThreads);
    hipLaunchKernelGGL(impair_rows_kernel, dim3((unsigned)(a.chunks * nrow)), dim3(kImpThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path(mode ? "phase_step" : "time_step");
    return SKDSP_OK;
}

}  // namespace skdsp
