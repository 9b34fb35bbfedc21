// pulse.hip -- the two filtering stages of a single-carrier BER loop over a frame set: pulse shaping, lfilter(b, 1, upsample(s, ns)) per row (sigsys.py:2163-2211,
// digitalcom.py:1676, 1821 of the reference), and the matched filter read at the symbol rate, lfilter(b, 1, x)[start::step] per row.  gfx950.  The plans, the
// arithmetic recipe and the per-thread functions are pulse_core.hpp, shared with tests/host/pulse_emul.cpp.
//
//   pulse_shape_rows_kernel   one workgroup per (row, tile of T symbols): the taps and T + H symbols staged in LDS, consecutive lanes produce consecutive
//                             output samples from their phase of the taps.  Bound by its stores: it writes ns times what it reads.
//   pulse_mf_rows_kernel      one workgroup per (row, tile of To outputs): the taps and the (To - 1) step + ntaps samples they read staged in LDS by phase
//                             (sample e in plane e mod step: what neighbouring lanes read lies side by side), each lane R outputs in registers over one
//                             walk of the taps.  Reads the input once, writes 1 / step of it.
// No atomics, plain vector loads and stores: two runs give the same bits, and those of the host forms.  Nothing outside a call's rows is read or written.
#include "skdsp_internal.hpp"
#include "pulse_core.hpp"

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
    __device__ __forceinline__ void st_f32(float *g, float v) const { *g = v; }
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
};

struct ShapeArgs {
    const void *x;
    void *y;
    const double *taps;
    pls::ShapePlan plan;
};

__global__ __launch_bounds__(pls::kThreads) void pulse_shape_rows_kernel(ShapeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double pulse_image[];
    const DevLds L = {pulse_image};
    const DevMem mem;
    const int64_t row = blockIdx.x / (uint32_t)a.plan.tiles, tile = blockIdx.x - row * a.plan.tiles;
    const char *x_row = static_cast<const char *>(a.x) + row * a.plan.x_stride * pls::elem_bytes(a.plan.dtype);
    char *y_row = static_cast<char *>(a.y) + row * a.plan.y_stride * pls::elem_bytes(a.plan.dtype);
    pls::shape_stage(mem, a.plan, a.taps, x_row, tile, (int)threadIdx.x, L);
    __syncthreads();
    pls::shape_outputs(mem, a.plan, y_row, tile, (int)threadIdx.x, L);
}

struct MfArgs {
    const void *x;
    void *y;
    const double *taps;
    pls::MfPlan plan;
};

template <int R, bool FMA, bool CPLX> __global__ __launch_bounds__(pls::kThreads) void pulse_mf_rows_kernel(MfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double pulse_image[];
    const DevLds L = {pulse_image};
    const DevMem mem;
    const int64_t row = blockIdx.x / (uint32_t)a.plan.tiles, tile = blockIdx.x - row * a.plan.tiles;
    const char *x_row = static_cast<const char *>(a.x) + row * a.plan.x_stride * pls::elem_bytes(a.plan.dtype);
    char *y_row = static_cast<char *>(a.y) + row * a.plan.y_stride * pls::elem_bytes(a.plan.dtype);
    pls::mf_stage(mem, a.plan, a.taps, x_row, tile, (int)threadIdx.x, L);
    __syncthreads();
    pls::mf_outputs<R, FMA, CPLX>(mem, a.plan, y_row, tile, (int)threadIdx.x, L);
}

struct PulseHandle : HandleBase {
    std::vector<double> taps_host;
    DevTable<double> taps;          // uploaded by the first launch: creating a handle and checking arguments need no device
};

template <class K, class A> int launch_tiles(K kern, const A &a, int64_t blocks, int lds_doubles, hipStream_t s)
{
    const size_t lds = (size_t)lds_doubles * sizeof(double);
    if (lds > 48 * 1024) SK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(pls::kThreads), lds, s, a);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

// the rows of x and of y as byte ranges: a call whose ranges meet is refused (in place is not supported: a tile reads what its neighbour writes)
bool ranges_meet(const void *x, int64_t x_stride, int64_t nx, const void *y, int64_t y_stride, int64_t ny, int64_t nrow, int esz)
{
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)((nrow - 1) * x_stride + nx) * esz, y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)((nrow - 1) * y_stride + ny) * esz;
    return x0 < y1 && y0 < x1;
}

int taps_ready(PulseHandle *h)
{
    std::lock_guard<std::mutex> lk(h->mu);
    return h->taps.dev ? SKDSP_OK : h->taps.upload(h->taps_host);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int pulse_create(const double *b, int ntaps, int dtype, HandleBase **out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "pulse_create: null out");
    SK_CHECK(b && ntaps >= 1, SKDSP_ERR_BADARG, "pulse_create: need at least one tap");
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "pulse_create: bad dtype %d", dtype);
    SK_CHECK(ntaps <= pls::kMaxTaps, SKDSP_ERR_UNSUPPORTED, "pulse_create: %d taps (the kernels take at most %d)", ntaps, pls::kMaxTaps);
    std::unique_ptr<PulseHandle> h(new PulseHandle());
    h->kind = H_PULSE;
    h->dtype = dtype;
    h->taps_host.assign(b, b + ntaps);
    *out = h.release();
    return SKDSP_OK;
}

int pulse_mf_out_len(int64_t n, int64_t start, int64_t step, int64_t *n_out)
{
    SK_CHECK(n_out, SKDSP_ERR_BADARG, "pulse_mf_out_len: null n_out");
    SK_CHECK(n >= 0 && start >= 0 && step >= 1 && n < pls::kMaxLen && start < pls::kMaxLen, SKDSP_ERR_BADARG, "pulse_mf_out_len: need 0 <= n, start < 2^40 and step >= 1");
    *n_out = pls::mf_out_len(n, start, step);
    return SKDSP_OK;
}

int pulse_shape_check(HandleBase *hb, int64_t n, int64_t nrow, int64_t ns, int64_t x_stride, int64_t y_stride)
{
    PulseHandle *h = static_cast<PulseHandle *>(hb);
    SK_CHECK(ns >= 1, SKDSP_ERR_BADARG, "pulse_shape: need ns >= 1 (got %lld)", (long long)ns);
    SK_CHECK(pls::served(ns, (int64_t)h->taps_host.size()), SKDSP_ERR_UNSUPPORTED, "pulse_shape: ns = %lld (the kernel takes 1 ... %d)", (long long)ns, pls::kMaxRate);
    pls::ShapePlan p;
    const char *why = pls::shape_plan_make(h->dtype, (int)h->taps_host.size(), ns, n, nrow, x_stride, y_stride, 0, 1.0, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "pulse_shape: %s (n = %lld, ns = %lld, x_stride = %lld, y_stride = %lld)", why, (long long)n, (long long)ns, (long long)x_stride,
             (long long)y_stride);
    return SKDSP_OK;
}

int pulse_shape_launch(HandleBase *hb, const void *x_dev, int64_t n, int64_t nrow, int64_t ns, int64_t x_stride, int64_t y_stride, int has_scale, double scale, void *y_dev,
                       hipStream_t s)
{
    int rc = pulse_shape_check(hb, n, nrow, ns, x_stride, y_stride);
    if (rc || n == 0 || nrow == 0) return rc;
    PulseHandle *h = static_cast<PulseHandle *>(hb);
    const int esz = (int)dtype_size(h->dtype);
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "pulse_shape: null pointer");
    SK_CHECK(elem_aligned(x_dev, y_dev, esz), SKDSP_ERR_BADARG, "pulse_shape: the rows must be aligned to their elements");
    SK_CHECK(!ranges_meet(x_dev, x_stride, n, y_dev, y_stride, n * ns, nrow, esz), SKDSP_ERR_BADARG, "pulse_shape: input and output overlap (in place is not supported)");
    if ((rc = taps_ready(h))) return rc;
    ShapeArgs a;
    pls::shape_plan_make(h->dtype, (int)h->taps_host.size(), ns, n, nrow, x_stride, y_stride, has_scale, scale, &a.plan);
    a.x = x_dev;
    a.y = y_dev;
    a.taps = h->taps.dev;
    if ((rc = launch_tiles(pulse_shape_rows_kernel, a, a.plan.tiles * nrow, a.plan.lds_doubles, s))) return rc;
    note_path("pulse_shape");
    return SKDSP_OK;
}

int pulse_mf_check(HandleBase *hb, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride)
{
    PulseHandle *h = static_cast<PulseHandle *>(hb);
    SK_CHECK(step >= 1, SKDSP_ERR_BADARG, "pulse_mf: need step >= 1 (got %lld)", (long long)step);
    SK_CHECK(pls::served(step, (int64_t)h->taps_host.size()), SKDSP_ERR_UNSUPPORTED, "pulse_mf: step = %lld (the kernel takes 1 ... %d)", (long long)step, pls::kMaxRate);
    pls::MfPlan p;
    const char *why = pls::mf_plan_make(h->dtype, (int)h->taps_host.size(), n, nrow, start, step, x_stride, y_stride, 0, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "pulse_mf: %s (n = %lld, start = %lld, step = %lld, x_stride = %lld, y_stride = %lld)", why, (long long)n, (long long)start,
             (long long)step, (long long)x_stride, (long long)y_stride);
    return SKDSP_OK;
}

int pulse_mf_launch(HandleBase *hb, const void *x_dev, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride, void *y_dev, hipStream_t s)
{
    int rc = pulse_mf_check(hb, n, nrow, start, step, x_stride, y_stride);
    if (rc || nrow == 0) return rc;
    PulseHandle *h = static_cast<PulseHandle *>(hb);
    const int variant = opt().pulse_mf_variant;
    MfArgs a;
    pls::mf_plan_make(h->dtype, (int)h->taps_host.size(), n, nrow, start, step, x_stride, y_stride, variant == 1, &a.plan);
    if (a.plan.n_out == 0) return SKDSP_OK;
    const int esz = (int)dtype_size(h->dtype);
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "pulse_mf: null pointer");
    SK_CHECK(elem_aligned(x_dev, y_dev, esz), SKDSP_ERR_BADARG, "pulse_mf: the rows must be aligned to their elements");
    SK_CHECK(!ranges_meet(x_dev, x_stride, n, y_dev, y_stride, a.plan.n_out, nrow, esz), SKDSP_ERR_BADARG, "pulse_mf: input and output overlap (in place is not supported)");
    if ((rc = taps_ready(h))) return rc;
    a.x = x_dev;
    a.y = y_dev;
    a.taps = h->taps.dev;
    const int64_t blocks = a.plan.tiles * nrow;
    const int lds = a.plan.lds_doubles, R = a.plan.R;
#define SK_MF(FMA, CPLX)                                                                                      \
    (R == 4 ? launch_tiles(pulse_mf_rows_kernel<4, FMA, CPLX>, a, blocks, lds, s)                            \
            : R == 2 ? launch_tiles(pulse_mf_rows_kernel<2, FMA, CPLX>, a, blocks, lds, s) : launch_tiles(pulse_mf_rows_kernel<1, FMA, CPLX>, a, blocks, lds, s))
    if (variant == 2)
        rc = a.plan.cplx ? SK_MF(true, true) : SK_MF(true, false);
    else
        rc = a.plan.cplx ? SK_MF(false, true) : SK_MF(false, false);
#undef SK_MF
    if (rc) return rc;
    note_path("pulse_mf");
    return SKDSP_OK;
}

}  // namespace skdsp
