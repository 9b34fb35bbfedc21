// symmap.hip -- Gray symbol mapping and demapping on the device: the symbol sequences of digitalcom.qam_gray_encode_bb / mpsk_gray_encode_bb
// (digitalcom.py:1584-1681, 1742-1826 of the reference) and digitalcom.qam_gray_decode / mpsk_gray_decode (digitalcom.py:1684-1739,
// 1829-1883) over the rows of a frame set.  gfx950.  The plans, the item geometry and the per-item functions are symmap_core.hpp, shared
// with tests/host/symmap_emul.cpp.
//
//   symmap_kernel          work item = (row, run of 2048 symbols), dealt over the whole grid.  The item's bits are staged into LDS in aligned
//                          16-byte chunks, a symbol's MSB-first word indexes the host's table (in LDS), the points leave as 16-byte stores
//                          that adjacent lanes place side by side.
//   symscale_kernel        the same items over the strided input x[start + k step]: a lane's (count, mean, M2) from two passes over its eight
//                          symbols, the lanes merged by a fixed tree in LDS, one partial per item into scratch.
//   symscale_merge_kernel  one workgroup per row: the row's partials dealt in contiguous shares, merged in order, then the same tree;
//                          r = 1 / (sqrt(M2 / n) c) as one float64.  No atomics anywhere: the same input gives the same bits.
//                          (symvar_launch: the same two kernels over rows of any dtype, real ones included, storing np.var = M2 / n -- the
//                          variance behind the channel's sigma and gain, channel.hip.)
//   symdemap_kernel        the same items: each symbol decided (qam_decide with the row's r read from device memory, or mpsk_index), its bits
//                          put into an LDS image laid out by the output run's alignment, which leaves in aligned 16-byte chunks.
// Nothing outside a row's bits, its symbols start + k step (k < n) and its output run is read or written.
#include "skdsp_internal.hpp"
#include "symmap_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *g) const { return *g; }
    __device__ __forceinline__ void st8(uint8_t *g, uint8_t v) const { *g = v; }
    __device__ __forceinline__ void in16(uint8_t *img, const uint8_t *g) const { *reinterpret_cast<uint4 *>(img) = *reinterpret_cast<const uint4 *>(g); }
    __device__ __forceinline__ void out16(uint8_t *g, const uint8_t *img) const { *reinterpret_cast<uint4 *>(g) = *reinterpret_cast<const uint4 *>(img); }
    __device__ __forceinline__ void st_c128(double *g, double re, double im) const { *reinterpret_cast<double2 *>(g) = make_double2(re, im); }
    __device__ __forceinline__ void st_c64(float *g, float re, float im) const { *reinterpret_cast<float2 *>(g) = make_float2(re, im); }
    __device__ __forceinline__ void st_c64x2(float *g, float r0, float i0, float r1, float i1) const { *reinterpret_cast<float4 *>(g) = make_float4(r0, i0, r1, i1); }
    __device__ __forceinline__ void ld_c64(const float *g, double *re, double *im) const
    {
        const float2 v = *reinterpret_cast<const float2 *>(g);
        *re = (double)v.x;
        *im = (double)v.y;
    }
    __device__ __forceinline__ double ld_f32(const float *g) const { return (double)*g; }
    __device__ __forceinline__ double ld_f64(const double *g) const { return *g; }
    __device__ __forceinline__ void ld_c128(const double *g, double *re, double *im) const
    {
        const double2 v = *reinterpret_cast<const double2 *>(g);
        *re = v.x;
        *im = v.y;
    }
};

// ------------------------------------------------------------------------------------------------------------------ map
struct MapArgs {
    const uint8_t *bits;
    void *y;
    int64_t bits_stride, y_stride;   // bytes / elements from row to row
    int64_t n;                       // symbols per row
    uint32_t items;                  // per row
    int c64;
    sym::MapPlan plan;
};

__global__ __launch_bounds__(sym::kThreads) void symmap_kernel(MapArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[sym::kImgBytes];
    __shared__ double tre[sym::kTab], tim[sym::kTab];
    const int t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < sym::kTab; ++i) {   // (constant indices: scalar loads of the arguments)
            tre[i] = a.plan.re[i];
            tim[i] = a.plan.im[i];
        }
    }
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int len = sym::item_len(a.n, it), bps = a.plan.bps;
    const uint8_t *gin = a.bits + row * a.bits_stride + sym::item_first(it) * bps;
    const int64_t e = row * a.y_stride + sym::item_first(it);
    void *gout = a.c64 ? (void *)(static_cast<float *>(a.y) + 2 * e) : (void *)(static_cast<double *>(a.y) + 2 * e);
    const DevMem mem;
    blk::stage_in(mem, gin, bps * len, img, t, sym::kThreads);
    __syncthreads();
    const sym::MapTab tab = {bps, a.plan.half, tre, tim};
    sym::map_store(mem, tab, img, blk::lead_of(gin), len, gout, a.c64, t, sym::kThreads);
}

// ------------------------------------------------------------------------------------------------------------------ scale
struct ScaleArgs {
    const void *x;
    int64_t x_stride, start, step, n;
    uint32_t items;
    int c64;
    int real = 0;         // 0: complex symbols (c64: complex64); 1: float32, 2: float64 values
    int var = 0;          // what r takes: 0 1 / (std c), 1 the variance M2 / n
    double c;
    sym::Moments *part;   // [nrow][items]
    double *r;            // [nrow]
};

__device__ __forceinline__ void tree_merge(sym::Moments *slot, int t)
{
    for (int off = sym::kThreads / 2; off >= 1; off >>= 1) {
        __syncthreads();
        sym::merge_step(slot, off, t);
    }
}

__global__ __launch_bounds__(sym::kThreads) void symscale_kernel(ScaleArgs a)
{
    __shared__ sym::Moments slot[sym::kThreads];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int len = sym::item_len(a.n, it);
    if (a.real) {
        const void *xrow = a.real == 1 ? (const void *)(static_cast<const float *>(a.x) + row * a.x_stride) : (const void *)(static_cast<const double *>(a.x) + row * a.x_stride);
        slot[t] = sym::scale_lane_real(DevMem(), xrow, a.start + sym::item_first(it) * a.step, a.step, a.real == 1, len, t);
    } else {
        const void *xrow = a.c64 ? (const void *)(static_cast<const float *>(a.x) + 2 * row * a.x_stride) : (const void *)(static_cast<const double *>(a.x) + 2 * row * a.x_stride);
        slot[t] = sym::scale_lane(DevMem(), xrow, a.start + sym::item_first(it) * a.step, a.step, a.c64, len, t);
    }
    tree_merge(slot, t);
    if (t == 0) a.part[blockIdx.x] = slot[0];
}

__global__ __launch_bounds__(sym::kThreads) void symscale_merge_kernel(ScaleArgs a)
{
    __shared__ sym::Moments slot[sym::kThreads];
    const int t = threadIdx.x;
    const sym::Moments *part = a.part + (int64_t)blockIdx.x * a.items;
    int64_t lo, hi;
    sym::share_of(a.items, t, sym::kThreads, &lo, &hi);
    sym::Moments m = sym::moments_none();
    for (int64_t j = lo; j < hi; ++j) m = sym::moments_merge(m, part[j]);
    slot[t] = m;
    tree_merge(slot, t);
    if (t == 0) a.r[blockIdx.x] = a.var ? sym::var_of(slot[0]) : sym::scale_of(slot[0], a.c);
}

// ------------------------------------------------------------------------------------------------------------------ demap
struct DemapArgs {
    const void *x;
    uint8_t *bits;
    int64_t x_stride, start, step, n, bits_stride;
    uint32_t items;
    int c64;
    const double *r;   // QAM: [nrow] on the device
    sym::DemapPlan plan;
};

__global__ __launch_bounds__(sym::kThreads) void symdemap_kernel(DemapArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[sym::kImgBytes];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int len = sym::item_len(a.n, it), bps = a.plan.bps;
    const void *xrow = a.c64 ? (const void *)(static_cast<const float *>(a.x) + 2 * row * a.x_stride) : (const void *)(static_cast<const double *>(a.x) + 2 * row * a.x_stride);
    uint8_t *gout = a.bits + row * a.bits_stride + sym::item_first(it) * bps;
    const double r = a.r ? a.r[row] : 1.0;
    const DevMem mem;
    sym::demap_lane(mem, a.plan, xrow, a.start + sym::item_first(it) * a.step, a.step, a.c64, len, r, img, blk::lead_of(gout), t);
    __syncthreads();
    blk::stage_out(mem, gout, bps * len, img, t, sym::kThreads);
}

bool grid_fits(int64_t items, int64_t nrow) { return items == 0 || nrow <= (((int64_t)1 << 31) - 1) / items; }

// the rules every call shares: sizes, the strided window, one launch
int common_check(const char *name, int64_t n, int64_t nrow, int dtype, int64_t x_stride, int64_t start, int64_t step)
{
    SK_CHECK(n >= 0 && nrow >= 0 && n < ((int64_t)1 << 40), SKDSP_ERR_BADARG, "%s: rows of 0 ... 2^40 - 1 symbols (n = %lld, nrow = %lld)", name, (long long)n, (long long)nrow);
    SK_CHECK(dtype == SKDSP_C64 || dtype == SKDSP_C128, SKDSP_ERR_BADARG, "%s: complex64 or complex128 symbols (dtype code %d)", name, dtype);
    SK_CHECK(x_stride >= 0 && start >= 0 && step >= 1 && start < ((int64_t)1 << 40) && step < ((int64_t)1 << 20), SKDSP_ERR_BADARG,
             "%s: need stride >= 0, 0 <= start < 2^40, 1 <= step < 2^20 (got %lld, %lld, %lld)", name, (long long)x_stride, (long long)start, (long long)step);
    SK_CHECK(grid_fits(sym::items_per_row(n), nrow), SKDSP_ERR_BADARG, "%s: %lld rows of %lld symbols in one launch", name, (long long)nrow, (long long)n);
    return SKDSP_OK;
}
bool sym_aligned(const void *p, int dtype) { return ((uintptr_t)p & (dtype == SKDSP_C64 ? 7u : 15u)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int sym_bits_per_symbol(int kind, int mod) { return sym::bps_of(kind, mod); }

int symmap_check(int kind, int mod, int64_t n, int64_t nrow, int dtype, int64_t bits_stride, int64_t y_stride)
{
    const char *why = sym::order_check(kind, mod);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "gray_map: %s", why);
    int rc = common_check("gray_map", n, nrow, dtype, y_stride, 0, 1);
    if (rc) return rc;
    SK_CHECK(bits_stride >= 0, SKDSP_ERR_BADARG, "gray_map: negative stride");
    return SKDSP_OK;
}

// nrow rows of bps n bytes 0 / 1 (bits_stride bytes apart) -> nrow rows of n points (y_stride elements apart); the table is the host's
int symmap_launch(const uint8_t *bits_dev, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab, int dtype,
                  void *y_dev, int64_t y_stride, hipStream_t s)
{
    int rc = symmap_check(kind, mod, n, nrow, dtype, bits_stride, y_stride);
    if (rc) return rc;
    MapArgs a;
    const char *why = sym::map_plan_make(kind, mod, tab_re, tab_im, ntab, &a.plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "gray_map: %s", why);
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(bits_dev && y_dev, SKDSP_ERR_BADARG, "gray_map: null pointer");
    SK_CHECK(sym_aligned(y_dev, dtype), SKDSP_ERR_BADARG, "gray_map: the output must be aligned to its element");
    a.bits = bits_dev;
    a.y = y_dev;
    a.bits_stride = bits_stride;
    a.y_stride = y_stride;
    a.n = n;
    a.items = (uint32_t)sym::items_per_row(n);
    a.c64 = dtype == SKDSP_C64;
    hipLaunchKernelGGL(symmap_kernel, dim3((unsigned)(a.items * nrow)), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("symmap");
    return SKDSP_OK;
}

int symscale_check(int mod, int64_t n, int64_t nrow, int dtype, int64_t x_stride, int64_t start, int64_t step)
{
    const char *why = sym::order_check(sym::kQam, mod);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "qam_scale: %s", why);
    return common_check("qam_scale", n, nrow, dtype, x_stride, start, step);
}
size_t symscale_scratch_bytes(int64_t n, int64_t nrow) { return (size_t)(sym::items_per_row(n) * nrow) * sizeof(sym::Moments); }

// r_dev[row] = 1 / (np.std(x[row, start + k step], k < n) c); scratch_dev: symscale_scratch_bytes(n, nrow) bytes, 8-byte aligned
int symscale_launch(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, void *scratch_dev,
                    double *r_dev, hipStream_t s)
{
    int rc = symscale_check(mod, n, nrow, dtype, x_stride, start, step);
    if (rc) return rc;
    if (nrow == 0) return SKDSP_OK;
    SK_CHECK(n >= 1, SKDSP_ERR_BADARG, "qam_scale: a row has no symbols");
    SK_CHECK(x_dev && r_dev && scratch_dev, SKDSP_ERR_BADARG, "qam_scale: null pointer");
    SK_CHECK(sym_aligned(x_dev, dtype) && ((uintptr_t)r_dev & 7) == 0, SKDSP_ERR_BADARG, "qam_scale: the pointers must be aligned to their elements");
    ScaleArgs a;
    a.x = x_dev;
    a.x_stride = x_stride;
    a.start = start;
    a.step = step;
    a.n = n;
    a.items = (uint32_t)sym::items_per_row(n);
    a.c64 = dtype == SKDSP_C64;
    a.c = c;
    a.part = static_cast<sym::Moments *>(scratch_dev);
    a.r = r_dev;
    hipLaunchKernelGGL(symscale_kernel, dim3((unsigned)(a.items * nrow)), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(symscale_merge_kernel, dim3((unsigned)nrow), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("symscale");
    return SKDSP_OK;
}

// var_dev[row] = np.var(x[row, k], k < n) = M2 / n of the same merge, for rows of any of the four dtypes (the channel's sigma and gain);
// scratch_dev as for symscale_launch
int symvar_launch(const void *x_dev, int64_t x_stride, int64_t n, int64_t nrow, int dtype, void *scratch_dev, double *var_dev, hipStream_t s)
{
    SK_CHECK(dtype >= SKDSP_F32 && dtype <= SKDSP_C128, SKDSP_ERR_BADARG, "row_var: float32, complex64, float64 or complex128 rows (dtype code %d)", dtype);
    SK_CHECK(n >= 1 && nrow >= 0 && n < ((int64_t)1 << 40) && x_stride >= 0, SKDSP_ERR_BADARG, "row_var: rows of 1 ... 2^40 - 1 elements (n = %lld, nrow = %lld)", (long long)n, (long long)nrow);
    SK_CHECK(grid_fits(sym::items_per_row(n), nrow), SKDSP_ERR_BADARG, "row_var: %lld rows of %lld elements in one launch", (long long)nrow, (long long)n);
    if (nrow == 0) return SKDSP_OK;
    SK_CHECK(x_dev && var_dev && scratch_dev, SKDSP_ERR_BADARG, "row_var: null pointer");
    SK_CHECK(((uintptr_t)x_dev & (dtype_size(dtype) - 1)) == 0 && ((uintptr_t)var_dev & 7) == 0, SKDSP_ERR_BADARG, "row_var: the pointers must be aligned to their elements");
    ScaleArgs a;
    a.x = x_dev;
    a.x_stride = x_stride;
    a.start = 0;
    a.step = 1;
    a.n = n;
    a.items = (uint32_t)sym::items_per_row(n);
    a.c64 = dtype == SKDSP_C64;
    a.real = dtype == SKDSP_F32 ? 1 : dtype == SKDSP_F64 ? 2 : 0;
    a.var = 1;
    a.c = 1.0;
    a.part = static_cast<sym::Moments *>(scratch_dev);
    a.r = var_dev;
    hipLaunchKernelGGL(symscale_kernel, dim3((unsigned)(a.items * nrow)), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(symscale_merge_kernel, dim3((unsigned)nrow), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("symvar");
    return SKDSP_OK;
}

int symdemap_check(int kind, int mod, int64_t n, int64_t nrow, int dtype, int64_t x_stride, int64_t start, int64_t step, int64_t bits_stride)
{
    const char *name = kind == sym::kQam ? "qam_demap" : "mpsk_demap";
    const char *why = sym::order_check(kind, mod);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "%s: %s", name, why);
    int rc = common_check(name, n, nrow, dtype, x_stride, start, step);
    if (rc) return rc;
    SK_CHECK(bits_stride >= 0, SKDSP_ERR_BADARG, "%s: negative stride", name);
    return SKDSP_OK;
}

// bits_dev[row, bps k ...] = the bits of symbol x[row, start + k step]; r_dev: the rows' scales (QAM), rot: np.exp(-1j pi / 4) (MPSK)
int symdemap_launch(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int kind, int mod, const double *r_dev,
                    double rot_re, double rot_im, uint8_t *bits_dev, int64_t bits_stride, hipStream_t s)
{
    int rc = symdemap_check(kind, mod, n, nrow, dtype, x_stride, start, step, bits_stride);
    if (rc) return rc;
    if (nrow == 0 || n == 0) return SKDSP_OK;
    const char *name = kind == sym::kQam ? "qam_demap" : "mpsk_demap";
    SK_CHECK(x_dev && bits_dev && (kind != sym::kQam || r_dev), SKDSP_ERR_BADARG, "%s: null pointer", name);
    SK_CHECK(sym_aligned(x_dev, dtype) && ((uintptr_t)r_dev & 7) == 0, SKDSP_ERR_BADARG, "%s: the pointers must be aligned to their elements", name);
    DemapArgs a;
    sym::demap_plan_make(kind, mod, rot_re, rot_im, &a.plan);
    a.x = x_dev;
    a.bits = bits_dev;
    a.x_stride = x_stride;
    a.start = start;
    a.step = step;
    a.n = n;
    a.bits_stride = bits_stride;
    a.items = (uint32_t)sym::items_per_row(n);
    a.c64 = dtype == SKDSP_C64;
    a.r = kind == sym::kQam ? r_dev : nullptr;
    hipLaunchKernelGGL(symdemap_kernel, dim3((unsigned)(a.items * nrow)), dim3(sym::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("symdemap");
    return SKDSP_OK;
}

}  // namespace skdsp
