// channel.hip -- the AWGN channel and the bit sources of the device-resident BER loops: sigsys.cpx_awgn / cpx_awgn2 (sigsys.py:2335-2454 of
// the reference), digitalcom.awgn_channel (digitalcom.py:1259-1281), sigsys.pn_gen (sigsys.py:1947-1980) and the encoders' random data bits,
// over the rows of a frame set.  gfx950.  The draw (Philox4x32-10, this project's own float64 ln and sincos), the plans, the chunk geometry
// and the per-chunk functions are channel_core.hpp, shared with tests/host/channel_emul.cpp.
//
//   awgn_kernel        y[r, i] = g[r] x[r, i] + sigma[r] z(seed, first_row + r, first + i): float32 / float64 (real z) or complex64 / complex128
//                      (complex z; a real x of the same precision is allowed).  The sum is formed in float64 and rounded once.
//   awgn_bits_kernel   bytes 0 / 1 in, the hard decision of 2 b - 1 + sigma z out as bytes: no float stream in between.
//   randbits_kernel    the bits of the tag-1 stream, one byte each.
//   pn_kernel          out[r, i] = period[(phase[r] + first + i) mod Q], one period of the sequence in device memory.
//   awgn_sigma_kernel  one thread per row: (g, sigma) of cpx_awgn / cpx_awgn2 from the row's variance, which symmap.hip's deterministic merge
//                      of partial moments wrote (symvar_launch).
// Every kernel walks flat (row, run of 1024 chunks) items; a chunk is an aligned 16 bytes of the OUTPUT, stored whole where it lies inside the
// row's run and component by component (byte by byte) at the run's two ends.  No LDS, no atomics: the value of an element depends on
// (seed, row, index) only.  Nothing outside a row's input window and output run is read or written; y == x (in place) is allowed.
#include "skdsp_internal.hpp"
#include "channel_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ double ld_f32(const float *g) const { return (double)*g; }
    __device__ __forceinline__ double ld_f64(const double *g) const { return *g; }
    __device__ __forceinline__ void st_f32(float *g, float v) const { *g = v; }
    __device__ __forceinline__ void st_f64(double *g, double v) const { *g = v; }
    __device__ __forceinline__ void ld_f32x4(const float *g, double *v) const
    {
        const float4 q = *reinterpret_cast<const float4 *>(g);
        v[0] = (double)q.x;
        v[1] = (double)q.y;
        v[2] = (double)q.z;
        v[3] = (double)q.w;
    }
    __device__ __forceinline__ void ld_f64x2(const double *g, double *v) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(g);
        v[0] = q.x;
        v[1] = q.y;
    }
    __device__ __forceinline__ void st_f32x4(float *g, float a, float b, float c, float d) const { *reinterpret_cast<float4 *>(g) = make_float4(a, b, c, d); }
    __device__ __forceinline__ void st_f64x2(double *g, double a, double b) const { *reinterpret_cast<double2 *>(g) = make_double2(a, b); }
    __device__ __forceinline__ uint8_t ld8(const uint8_t *g) const { return *g; }
    __device__ __forceinline__ void st8(uint8_t *g, uint8_t v) const { *g = v; }
    __device__ __forceinline__ uint8_t ld_tab(const uint8_t *tab, int i) const { return tab[i]; }
    __device__ __forceinline__ void ld_b16(const uint8_t *g, chan::Bytes16 &v) const
    {
        const uint4 q = *reinterpret_cast<const uint4 *>(g);
        v.w[0] = q.x;
        v.w[1] = q.y;
        v.w[2] = q.z;
        v.w[3] = q.w;
    }
    __device__ __forceinline__ void st_b16(uint8_t *g, const chan::Bytes16 &v) const { *reinterpret_cast<uint4 *>(g) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]); }
};

// ------------------------------------------------------------------------------------------------------------------ awgn
struct AwgnArgs {
    const void *x;
    void *y;
    int64_t x_stride, y_stride;            // elements from row to row
    uint32_t items;                        // per row
    const double *g_dev, *sigma_dev;       // [nrow] on the device, or null: the scalars
    double g, sigma;
    chan::AwgnPlan plan;
};

__global__ __launch_bounds__(chan::kThreads) void awgn_kernel(AwgnArgs a)
{
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int64_t ye = chan::awgn_comp_bytes(a.plan) * (a.plan.y_cpx ? 2 : 1), xe = chan::awgn_comp_bytes(a.plan) * (a.plan.x_cpx ? 2 : 1);
    const void *x = static_cast<const char *>(a.x) + row * a.x_stride * xe;
    void *y = static_cast<char *>(a.y) + row * a.y_stride * ye;
    const double g = a.g_dev ? a.g_dev[row] : a.g, sigma = a.sigma_dev ? a.sigma_dev[row] : a.sigma;
    const DevMem mem;
    for (int u = 0; u < chan::kChunkRun; ++u) chan::awgn_chunk(mem, a.plan, (uint32_t)row, x, y, g, sigma, chan::lane_chunk(it, t, u));
}

// ------------------------------------------------------------------------------------------------------------------ bits
struct BitsArgs {
    const uint8_t *x;                      // awgn_bits: the bits in
    uint8_t *y;
    int64_t x_stride, y_stride;            // bytes from row to row
    uint32_t items;
    const double *sigma_dev;
    double sigma;
    chan::BitsPlan plan;
};

__global__ __launch_bounds__(chan::kThreads) void awgn_bits_kernel(BitsArgs a)
{
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const double sigma = a.sigma_dev ? a.sigma_dev[row] : a.sigma;
    const DevMem mem;
    for (int u = 0; u < chan::kChunkRun; ++u)
        chan::awgn_bits_chunk(mem, a.plan, (uint32_t)row, a.x + row * a.x_stride, a.y + row * a.y_stride, sigma, chan::lane_chunk(it, t, u));
}

__global__ __launch_bounds__(chan::kThreads) void randbits_kernel(BitsArgs a)
{
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const DevMem mem;
    for (int u = 0; u < chan::kChunkRun; ++u) chan::randbits_chunk(mem, a.plan, (uint32_t)row, a.y + row * a.y_stride, chan::lane_chunk(it, t, u));
}

struct PnArgs {
    const uint8_t *period;
    const int64_t *phases;                 // [nrow] on the device, or null: 0
    uint8_t *y;
    int64_t y_stride;
    uint32_t items;
    chan::PnPlan plan;
};

__global__ __launch_bounds__(chan::kThreads) void pn_kernel(PnArgs a)
{
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int64_t phase = a.phases ? a.phases[row] : 0;
    const DevMem mem;
    for (int u = 0; u < chan::kChunkRun; ++u) chan::pn_chunk(mem, a.plan, a.period, phase, a.y + row * a.y_stride, chan::lane_chunk(it, t, u));
}

// ------------------------------------------------------------------------------------------------------------------ sigma and gain
struct SigmaArgs {
    double *g, *sigma;                     // sigma[row] arrives holding the row's variance
    int64_t nrow;
    int mode;
    double ns, p, var_w;
};

__global__ __launch_bounds__(chan::kThreads) void awgn_sigma_kernel(SigmaArgs a)
{
    const int64_t row = (int64_t)blockIdx.x * chan::kThreads + threadIdx.x;
    if (row >= a.nrow) return;
    double g, sigma;
    chan::sigma_gain(a.mode, a.sigma[row], a.ns, a.p, a.var_w, &g, &sigma);
    a.g[row] = g;
    a.sigma[row] = sigma;
}

bool grid_fits(int64_t items, int64_t nrow) { return items == 0 || nrow <= (((int64_t)1 << 31) - 1) / items; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int awgn_check(int x_dtype, int y_dtype, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, int64_t first, int64_t first_row)
{
    chan::AwgnPlan p;
    const char *why = chan::awgn_plan_make(x_dtype, y_dtype, 0, first, first_row, n, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "awgn: %s", why);
    SK_CHECK(nrow >= 0 && x_stride >= 0 && y_stride >= 0 && first_row + nrow <= ((int64_t)1 << 32), SKDSP_ERR_BADARG, "awgn: need nrow >= 0, strides >= 0, first_row + nrow <= 2^32");
    SK_CHECK(grid_fits(chan::items_per_row(chan::awgn_row_bytes(p), false), nrow), SKDSP_ERR_BADARG, "awgn: %lld rows of %lld elements in one launch", (long long)nrow, (long long)n);
    return SKDSP_OK;
}

// y[r, i] = g[r] x[r, i] + sigma[r] z(seed, first_row + r, first + i); g_dev / sigma_dev: the rows' values on the device, or null for the scalars
int awgn_launch(const void *x_dev, int64_t x_stride, int x_dtype, void *y_dev, int64_t y_stride, int y_dtype, int64_t n, int64_t nrow, const double *g_dev,
                const double *sigma_dev, double g, double sigma, uint64_t seed, int64_t first, int64_t first_row, hipStream_t s)
{
    int rc = awgn_check(x_dtype, y_dtype, n, nrow, x_stride, y_stride, first, first_row);
    if (rc) return rc;
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "awgn: null pointer");
    SK_CHECK(((uintptr_t)x_dev & (dtype_size(x_dtype) - 1)) == 0 && ((uintptr_t)y_dev & (dtype_size(y_dtype) - 1)) == 0 && ((uintptr_t)g_dev & 7) == 0 &&
                 ((uintptr_t)sigma_dev & 7) == 0,
             SKDSP_ERR_BADARG, "awgn: the pointers must be aligned to their elements");
    AwgnArgs a;
    chan::awgn_plan_make(x_dtype, y_dtype, seed, first, first_row, n, &a.plan);
    a.x = x_dev;
    a.y = y_dev;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.items = (uint32_t)chan::items_per_row(chan::awgn_row_bytes(a.plan), chan::rows_aligned16(y_dev, y_stride * (int64_t)dtype_size(y_dtype)));
    a.g_dev = g_dev;
    a.sigma_dev = sigma_dev;
    a.g = g;
    a.sigma = sigma;
    hipLaunchKernelGGL(awgn_kernel, dim3((unsigned)(a.items * nrow)), dim3(chan::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("awgn");
    return SKDSP_OK;
}

int chanbits_check(const char *name, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, int64_t first, int64_t first_row)
{
    chan::BitsPlan p;
    const char *why = chan::bits_plan_make(0, first, first_row, n, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "%s: %s", name, why);
    SK_CHECK(nrow >= 0 && x_stride >= 0 && y_stride >= 0 && first_row + nrow <= ((int64_t)1 << 32), SKDSP_ERR_BADARG, "%s: need nrow >= 0, strides >= 0, first_row + nrow <= 2^32", name);
    SK_CHECK(grid_fits(chan::items_per_row(n, false), nrow), SKDSP_ERR_BADARG, "%s: %lld rows of %lld bits in one launch", name, (long long)nrow, (long long)n);
    return SKDSP_OK;
}

// x_dev null: the random bits of the tag-1 stream; else the hard decisions of x's bits through the channel
int chanbits_launch(const uint8_t *x_dev, int64_t x_stride, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, const double *sigma_dev, double sigma, uint64_t seed,
                    int64_t first, int64_t first_row, int random, hipStream_t s)
{
    const char *name = random ? "random_bits" : "awgn_bits";
    int rc = chanbits_check(name, n, nrow, x_stride, y_stride, first, first_row);
    if (rc) return rc;
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(y_dev && (random || x_dev), SKDSP_ERR_BADARG, "%s: null pointer", name);
    SK_CHECK(((uintptr_t)sigma_dev & 7) == 0, SKDSP_ERR_BADARG, "%s: sigma must be aligned to 8 bytes", name);
    BitsArgs a;
    chan::bits_plan_make(seed, first, first_row, n, &a.plan);
    a.x = x_dev;
    a.y = y_dev;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.items = (uint32_t)chan::items_per_row(n, chan::rows_aligned16(y_dev, y_stride));
    a.sigma_dev = sigma_dev;
    a.sigma = sigma;
    if (random) hipLaunchKernelGGL(randbits_kernel, dim3((unsigned)(a.items * nrow)), dim3(chan::kThreads), 0, s, a);
    else hipLaunchKernelGGL(awgn_bits_kernel, dim3((unsigned)(a.items * nrow)), dim3(chan::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path(random ? "randbits" : "awgn_bits");
    return SKDSP_OK;
}

int pn_check(int Q, int64_t n, int64_t nrow, int64_t y_stride, int64_t first)
{
    chan::PnPlan p;
    const char *why = chan::pn_plan_make(Q, first, n, &p);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "pn: %s", why);
    SK_CHECK(nrow >= 0 && y_stride >= 0, SKDSP_ERR_BADARG, "pn: need nrow >= 0, stride >= 0");
    SK_CHECK(grid_fits(chan::items_per_row(n, false), nrow), SKDSP_ERR_BADARG, "pn: %lld rows of %lld bits in one launch", (long long)nrow, (long long)n);
    return SKDSP_OK;
}

// y[r, i] = period[(phases[r] + first + i) mod Q]; period_dev: Q bytes, phases_dev: nrow int64 >= 0 (or null: 0), both on the device
int pn_launch(const uint8_t *period_dev, int Q, const int64_t *phases_dev, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, int64_t first, hipStream_t s)
{
    int rc = pn_check(Q, n, nrow, y_stride, first);
    if (rc) return rc;
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(period_dev && y_dev, SKDSP_ERR_BADARG, "pn: null pointer");
    SK_CHECK(((uintptr_t)phases_dev & 7) == 0, SKDSP_ERR_BADARG, "pn: the phases must be aligned to 8 bytes");
    PnArgs a;
    chan::pn_plan_make(Q, first, n, &a.plan);
    a.period = period_dev;
    a.phases = phases_dev;
    a.y = y_dev;
    a.y_stride = y_stride;
    a.items = (uint32_t)chan::items_per_row(n, chan::rows_aligned16(y_dev, y_stride));
    hipLaunchKernelGGL(pn_kernel, dim3((unsigned)(a.items * nrow)), dim3(chan::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("pn");
    return SKDSP_OK;
}

// (g, sigma)[row] of cpx_awgn (mode 0) / cpx_awgn2 (mode 1) from sigma_dev[row] = the row's variance (symvar_launch wrote it)
int awgn_sigma_launch(int mode, double ns, double p, double var_w, int64_t nrow, double *g_dev, double *sigma_dev, hipStream_t s)
{
    SK_CHECK(mode == chan::kSigmaAwgn || mode == chan::kSigmaAwgn2, SKDSP_ERR_BADARG, "awgn_sigma: mode 0 (cpx_awgn) or 1 (cpx_awgn2)");
    if (nrow == 0) return SKDSP_OK;
    SK_CHECK(g_dev && sigma_dev && ((uintptr_t)g_dev & 7) == 0 && ((uintptr_t)sigma_dev & 7) == 0, SKDSP_ERR_BADARG, "awgn_sigma: null or misaligned pointer");
    SigmaArgs a = {g_dev, sigma_dev, nrow, mode, ns, p, var_w};
    hipLaunchKernelGGL(awgn_sigma_kernel, dim3((unsigned)((nrow + chan::kThreads - 1) / chan::kThreads)), dim3(chan::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("awgn_sigma");
    return SKDSP_OK;
}

}  // namespace skdsp
