// ofdm.hip -- OFDM modulation and demodulation over the rows of a frame set: digitalcom.ofdm_tx / ofdm_rx / chan_est_equalize
// (digitalcom.py:1322-1547 of the reference; mux_pilot_blocks is index arithmetic in the transmitter's loader).  gfx950.  The argument
// rules, the carrier map, the plans and the per-thread phases are ofdm_core.hpp, shared with tests/host/ofdm_emul.cpp.
//
//   ofdm_tx_kernel        a work item is a group of NB consecutive (muxed) symbols of one row; a workgroup walks items.  Loader = carrier map
//                         (data / 1 of a pilot / 0), read conjugated; psd_core.hpp's float64 FFT in LDS; the store reads LDS at pos_of((m - ncp)
//                         mod nc), conjugates and scales by 1 / nc: the group leaves as one contiguous run of NB (nc + ncp) samples.
//   ofdm_rx_kernel        the same walk over received symbols: loader x[k stride + off + n], the nf picked bins out of LDS at pos_of(bin(c)),
//                         pilots to the pilot buffer, data rows to their compacted index, divided by the table where there is one.
//   ofdm_chanest_kernel   one thread per (row, carrier), adjacent lanes on adjacent carriers: the recursion over the row's pilots, in order.
//   ofdm_equalize_kernel  one thread per data element: the division by estimate k / npb, or by the table.
// float64 butterflies, twiddles and LDS image for both dtypes; a complex64 result is rounded once, at its store.  No atomics: the result is
// bit-identical from run to run.  An idle segment of a row's last group transforms zeros, takes part in every barrier and touches no global
// memory; nothing outside a row's input window and output run is read or written.  In place is not offered.
#include <math.h>
#include "skdsp_internal.hpp"
#include "ofdm_core.hpp"

namespace skdsp {
namespace {

using ofdm::cx;
using ofdm::kThreads;

struct DevMem {
    __device__ __forceinline__ cx<double> ld(const float *g) const
    {
        const float2 q = *reinterpret_cast<const float2 *>(g);
        return cx<double>{(double)q.x, (double)q.y};
    }
    __device__ __forceinline__ cx<double> ld(const double *g) const
    {
        const double2 q = *reinterpret_cast<const double2 *>(g);
        return cx<double>{q.x, q.y};
    }
    __device__ __forceinline__ cx<double> ld_tab(const cx<double> *tab, int i) const { return tab[i]; }
    __device__ __forceinline__ void st(float *g, cx<double> v) const { *reinterpret_cast<float2 *>(g) = make_float2((float)v.x, (float)v.y); }
    __device__ __forceinline__ void st(double *g, cx<double> v) const { *reinterpret_cast<double2 *>(g) = make_double2(v.x, v.y); }
    __device__ __forceinline__ void st2(float *g, cx<double> a, cx<double> b) const
    {
        *reinterpret_cast<float4 *>(g) = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
    }
};

// passes 1 .. of the transform on the group's images, a barrier after each
template <int LOG2N> __device__ __forceinline__ void transform_rest(int tid, const cx<double> *tw, cx<double> *work)
{
    typedef ofdm::Core<LOG2N> C;
    cx<double> *img = work + (tid / C::TS) * C::N;
    const int t = tid % C::TS;
    __syncthreads();
    SK_UNROLL
    for (int s = 1; s < C::NSTORE; ++s) {
        C::mid(s, t, tw, img);
        __syncthreads();
    }
    C::last_store(t, img);
    __syncthreads();
}

template <typename S, int LOG2N>
__global__ __launch_bounds__(kThreads) void ofdm_tx_kernel(const S *__restrict__ x, S *__restrict__ y, ofdm::TxPlan p, int64_t items,
                                                           const cx<double> *__restrict__ tw)
{
    typedef ofdm::Core<LOG2N> C;
    __shared__ __attribute__((aligned(16))) cx<double> work[C::NB * C::N];
    const int tid = threadIdx.x;
    const DevMem mem;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t row = it / p.groups, j0 = (it - row * p.groups) * C::NB;
        ofdm::tx_first<S, LOG2N>(mem, p, x + 2 * row * p.x_stride, j0, tid, tw, work);
        transform_rest<LOG2N>(tid, tw, work);
        ofdm::tx_store<S, LOG2N>(mem, p, y + 2 * row * p.y_stride, j0, tid, work);
        __syncthreads();   // the next item's first pass overwrites the images
    }
}

template <typename SI, typename SO, int LOG2N>
__global__ __launch_bounds__(kThreads) void ofdm_rx_kernel(const SI *__restrict__ x, SO *__restrict__ z, double *__restrict__ pil,
                                                           const cx<double> *__restrict__ hht, ofdm::RxPlan p, int64_t items,
                                                           const cx<double> *__restrict__ tw)
{
    typedef ofdm::Core<LOG2N> C;
    __shared__ __attribute__((aligned(16))) cx<double> work[C::NB * C::N];
    const int tid = threadIdx.x;
    const DevMem mem;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t row = it / p.groups, k0 = (it - row * p.groups) * C::NB;
        ofdm::rx_first<SI, LOG2N>(mem, p, x + 2 * row * p.x_stride, k0, tid, tw, work);
        transform_rest<LOG2N>(tid, tw, work);
        ofdm::rx_store<SO, LOG2N>(mem, p, z + 2 * row * p.z_stride, pil + 2 * row * p.npilot * p.nf, hht, k0, tid, work);
        __syncthreads();
    }
}

struct EstArgs {
    int64_t src_stride, pitch, npilot;   // elements from row to row and from pilot to pilot of src
    int nf, bpr;                         // blocks per row
    double alpha;
};

template <typename SI>
__global__ __launch_bounds__(kThreads) void ofdm_chanest_kernel(const SI *src, double *est, double *__restrict__ h, EstArgs a)
{
    const int64_t row = blockIdx.x / a.bpr;
    const int c = (int)(blockIdx.x - row * a.bpr) * kThreads + threadIdx.x;
    if (c >= a.nf) return;
    const DevMem mem;
    ofdm::chanest_item<SI>(mem, src + 2 * row * a.src_stride, a.pitch, a.npilot, a.nf, c, a.alpha, est + 2 * row * a.npilot * a.nf, h + 2 * row * a.nf);
}

struct EqArgs {
    int64_t src_stride, out_stride, npilot, ndata, bpr;
    int nf, npb, compact;
};

template <typename SI, typename SO>
__global__ __launch_bounds__(kThreads) void ofdm_equalize_kernel(const SI *__restrict__ src, const double *__restrict__ est,
                                                                 const cx<double> *__restrict__ hht, SO *__restrict__ out, EqArgs a)
{
    const int64_t row = blockIdx.x / a.bpr, e = (blockIdx.x - row * a.bpr) * kThreads + threadIdx.x;
    if (e >= a.ndata * a.nf) return;
    const DevMem mem;
    ofdm::equalize_item<SI, SO>(mem, src + 2 * row * a.src_stride, a.compact, est + 2 * row * a.npilot * a.nf, hht, a.nf, a.npb, e, out + 2 * row * a.out_stride);
}

// ---- the twiddles exp(-2 pi j i / nc) in float64, kept per (device, log2 nc).  Never destroyed: the tables own device memory, and a free
// during static destruction -- after the runtime has torn down -- hangs or aborts the exit of the process.
struct TwTab {
    int device, log2n;
    DevTable<double> tw;
};
std::mutex g_tw_mu;
std::vector<TwTab> &g_tw = *new std::vector<TwTab>();

int twiddles_for(int log2n, const cx<double> **out)
{
    std::lock_guard<std::mutex> lk(g_tw_mu);
    const int dev = ctx().device;
    for (TwTab &t : g_tw)
        if (t.device == dev && t.log2n == log2n) {
            *out = reinterpret_cast<const cx<double> *>(t.tw.dev);
            return SKDSP_OK;
        }
    const int N = 1 << log2n;
    std::vector<double> tw(2 * (size_t)N);
    const double kTwoPi = 6.283185307179586476925286766559;
    for (int i = 0; i < N; ++i) {
        tw[2 * i] = cos(kTwoPi * i / N);
        tw[2 * i + 1] = -sin(kTwoPi * i / N);
    }
    TwTab t;
    t.device = dev;
    t.log2n = log2n;
    const int rc = t.tw.upload(tw);
    if (rc) return rc;
    *out = reinterpret_cast<const cx<double> *>(t.tw.dev);
    g_tw.push_back(std::move(t));
    return SKDSP_OK;
}

int64_t walk_grid(int64_t items)
{
    const int64_t g = 8 * (int64_t)ctx().num_cus;
    return items < g ? items : g;
}

template <typename S, int LOG2N>
void tx_launch_one(const void *x, void *y, const ofdm::TxPlan &p, int64_t items, const cx<double> *tw, hipStream_t s)
{
    hipLaunchKernelGGL((ofdm_tx_kernel<S, LOG2N>), dim3((unsigned)walk_grid(items)), dim3(kThreads), 0, s, (const S *)x, (S *)y, p, items, tw);
}
template <typename SI, typename SO, int LOG2N>
void rx_launch_one(const void *x, void *z, double *pil, const cx<double> *hht, const ofdm::RxPlan &p, int64_t items, const cx<double> *tw, hipStream_t s)
{
    hipLaunchKernelGGL((ofdm_rx_kernel<SI, SO, LOG2N>), dim3((unsigned)walk_grid(items)), dim3(kThreads), 0, s, (const SI *)x, (SO *)z, pil, hht, p, items, tw);
}
#define SK_OFDM_LOG2(call, ...)                      \
    switch (log2n) {                                 \
    case 6: call<__VA_ARGS__, 6> args; break;        \
    case 7: call<__VA_ARGS__, 7> args; break;        \
    case 8: call<__VA_ARGS__, 8> args; break;        \
    case 9: call<__VA_ARGS__, 9> args; break;        \
    case 10: call<__VA_ARGS__, 10> args; break;      \
    case 11: call<__VA_ARGS__, 11> args; break;      \
    default: call<__VA_ARGS__, 12> args; break;      \
    }

bool rows_fit(int64_t need, int64_t stride, int64_t nrow) { return stride >= 0 && (nrow <= 1 || stride >= need); }
constexpr int64_t kMaxElems = (int64_t)1 << 40;   // per row: keeps every index product inside int64

// scratch: [the table: nf complex128, to 256 bytes][pilots / estimates: nrow npilot nf complex128][raw data rows: nrow ndata nf complex128]
size_t tab_bytes(int nf) { return ((size_t)nf * 16 + 255) / 256 * 256; }

template <typename SI> int chanest_run(const void *src, int64_t src_stride, int64_t pitch, int64_t npilot, int64_t nrow, int nf, double alpha, double *est, double *h, hipStream_t s)
{
    EstArgs a;
    a.src_stride = src_stride;
    a.pitch = pitch;
    a.npilot = npilot;
    a.nf = nf;
    a.bpr = (nf + kThreads - 1) / kThreads;
    a.alpha = alpha;
    SK_CHECK(nrow <= (((int64_t)1 << 31) - 1) / a.bpr, SKDSP_ERR_BADARG, "ofdm: %lld rows in one launch", (long long)nrow);
    hipLaunchKernelGGL((ofdm_chanest_kernel<SI>), dim3((unsigned)(a.bpr * nrow)), dim3(kThreads), 0, s, (const SI *)src, est, h, a);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

template <typename SI, typename SO>
int equalize_run(const void *src, int64_t src_stride, int compact, const double *est, const cx<double> *hht, int64_t npilot, int64_t ndata, int64_t nrow, int nf, int npb,
                 void *out, int64_t out_stride, hipStream_t s)
{
    EqArgs a;
    a.src_stride = src_stride;
    a.out_stride = out_stride;
    a.npilot = npilot;
    a.ndata = ndata;
    a.bpr = (ndata * nf + kThreads - 1) / kThreads;
    a.nf = nf;
    a.npb = npb;
    a.compact = compact;
    if (a.bpr == 0) return SKDSP_OK;
    SK_CHECK(nrow <= (((int64_t)1 << 31) - 1) / a.bpr, SKDSP_ERR_BADARG, "ofdm: %lld rows of %lld data symbols in one launch", (long long)nrow, (long long)ndata);
    hipLaunchKernelGGL((ofdm_equalize_kernel<SI, SO>), dim3((unsigned)(a.bpr * nrow)), dim3(kThreads), 0, s, (const SI *)src, est, hht, (SO *)out, a);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
int ofdm_tx_check(int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, int64_t x_stride, int64_t y_stride)
{
    SK_CHECK(dtype == SKDSP_C64 || dtype == SKDSP_C128, SKDSP_ERR_BADARG, "ofdm_tx: complex64 or complex128 rows (dtype code %d)", dtype);
    const char *why = ofdm::shape_why(nf, nc, npb, ncp, 0, 0);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "ofdm_tx: %s (nf = %d, nc = %d, npb = %d, ncp = %d)", why, nf, nc, npb, ncp);
    SK_CHECK(nsym >= 0 && nrow >= 0 && nsym <= kMaxElems / (2 * nc), SKDSP_ERR_BADARG, "ofdm_tx: %lld symbols in %lld rows", (long long)nsym, (long long)nrow);
    const int64_t T = ofdm::tx_symbols(nsym, npb);
    SK_CHECK(rows_fit(nsym * nf, x_stride, nrow) && rows_fit(T * (nc + (cp ? ncp : 0)), y_stride, nrow), SKDSP_ERR_BADARG, "ofdm_tx: the rows overlap (strides %lld, %lld)",
             (long long)x_stride, (long long)y_stride);
    return SKDSP_OK;
}

// y[r]: the T (nc + ncp) samples of row r's nsym data symbols of nf carriers each (T = nsym without pilots)
int ofdm_tx_launch(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y_dev, int64_t y_stride,
                   hipStream_t s)
{
    int rc = ofdm_tx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, x_stride, y_stride);
    if (rc) return rc;
    ofdm::TxPlan p;
    ofdm::tx_plan_make(nsym, nf, nc, npb, cp, ncp, x_stride, y_stride, &p);
    if (nrow == 0 || p.T == 0) return SKDSP_OK;
    const size_t esz = dtype_size(dtype);
    SK_CHECK(y_dev && (x_dev || nsym == 0), SKDSP_ERR_BADARG, "ofdm_tx: null pointer");
    SK_CHECK((((uintptr_t)x_dev | (uintptr_t)y_dev) & (esz - 1)) == 0, SKDSP_ERR_BADARG, "ofdm_tx: the pointers must be aligned to their elements");
    SK_CHECK(nrow <= (((int64_t)1 << 62) / p.groups), SKDSP_ERR_BADARG, "ofdm_tx: %lld rows in one launch", (long long)nrow);
    const int log2n = ofdm::log2_of(nc);
    const cx<double> *tw = nullptr;
    if ((rc = twiddles_for(log2n, &tw))) return rc;
    const int64_t items = p.groups * nrow;
#define args (x_dev, y_dev, p, items, tw, s)
    if (dtype == SKDSP_C64) {
        SK_OFDM_LOG2(tx_launch_one, float)
    } else {
        SK_OFDM_LOG2(tx_launch_one, double)
    }
#undef args
    SK_HIP(hipGetLastError());
    note_path("ofdm_tx");
    return SKDSP_OK;
}

int ofdm_rx_check(int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, int has_table, int64_t x_stride, int64_t z_stride)
{
    SK_CHECK(dtype == SKDSP_C64 || dtype == SKDSP_C128, SKDSP_ERR_BADARG, "ofdm_rx: complex64 or complex128 rows (dtype code %d)", dtype);
    const char *why = ofdm::shape_why(nf, nc, npb, ncp, 1, has_table);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "ofdm_rx: %s (nf = %d, nc = %d, npb = %d, ncp = %d)", why, nf, nc, npb, ncp);
    SK_CHECK(nsym >= 0 && nrow >= 0 && nsym <= kMaxElems / (2 * nc), SKDSP_ERR_BADARG, "ofdm_rx: %lld symbols in %lld rows", (long long)nsym, (long long)nrow);
    const int64_t ndata = nsym - ofdm::rx_pilots(nsym, npb);
    SK_CHECK(rows_fit(nsym * (cp ? nc + ncp : nc), x_stride, nrow) && rows_fit(ndata * nf, z_stride, nrow), SKDSP_ERR_BADARG, "ofdm_rx: the rows overlap (strides %lld, %lld)",
             (long long)x_stride, (long long)z_stride);
    return SKDSP_OK;
}

// the table, and one complex128 per (row, symbol, carrier): the pilots and the raw data rows together
size_t ofdm_scratch_bytes(int64_t nsym, int64_t nrow, int nf) { return tab_bytes(nf) + (size_t)nrow * (size_t)nsym * (size_t)nf * 16 + 256; }

// z[r]: the ndata nf equalised carriers of row r's nsym received symbols; h[r]: the row's last estimate (npb > 0 only; nf complex128).
// hht_host: the known channel on the filled carriers (nf complex128 on the host) or null
int ofdm_rx_launch(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                   const double *hht_host, void *scratch_dev, void *z_dev, int64_t z_stride, void *h_dev, hipStream_t s)
{
    int rc = ofdm_rx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, hht_host != nullptr, x_stride, z_stride);
    if (rc) return rc;
    if (nrow == 0 || nsym == 0) return SKDSP_OK;
    const size_t esz = dtype_size(dtype);
    SK_CHECK(x_dev && scratch_dev && (npb <= 0 || h_dev), SKDSP_ERR_BADARG, "ofdm_rx: null pointer");
    SK_CHECK((((uintptr_t)x_dev | (uintptr_t)z_dev) & (esz - 1)) == 0 && ((uintptr_t)h_dev & 15) == 0 && ((uintptr_t)scratch_dev & 255) == 0, SKDSP_ERR_BADARG,
             "ofdm_rx: the pointers must be aligned to their elements");
    const bool use_tab = hht_host && npb != 0, raw = npb > 0 && !hht_host;
    char *sc = static_cast<char *>(scratch_dev);
    cx<double> *hht = use_tab ? reinterpret_cast<cx<double> *>(sc) : nullptr;
    double *pil = reinterpret_cast<double *>(sc + tab_bytes(nf));
    ofdm::RxPlan p;
    ofdm::rx_plan_make(nsym, nf, nc, npb, cp, ncp, x_stride, z_stride, &p);
    double *rawz = pil + 2 * (size_t)nrow * (size_t)p.npilot * nf;
    if (raw) p.z_stride = p.ndata * nf;
    SK_CHECK(z_dev || p.ndata == 0, SKDSP_ERR_BADARG, "ofdm_rx: null pointer");
    if (use_tab) SK_HIP(hipMemcpyAsync(hht, hht_host, (size_t)nf * 16, hipMemcpyHostToDevice, s));
    const int log2n = ofdm::log2_of(nc);
    const cx<double> *tw = nullptr;
    if ((rc = twiddles_for(log2n, &tw))) return rc;
    const int64_t items = p.groups * nrow;
    void *zk = raw ? (void *)rawz : z_dev;
#define args (x_dev, zk, pil, hht, p, items, tw, s)
    if (dtype == SKDSP_C128) {
        SK_OFDM_LOG2(rx_launch_one, double, double)
    } else if (raw) {
        SK_OFDM_LOG2(rx_launch_one, float, double)
    } else {
        SK_OFDM_LOG2(rx_launch_one, float, float)
    }
#undef args
    SK_HIP(hipGetLastError());
    note_path("ofdm_rx");
    if (npb > 0) {
        if ((rc = chanest_run<double>(pil, p.npilot * nf, nf, p.npilot, nrow, nf, alpha, pil, (double *)h_dev, s))) return rc;
        if (raw) {
            rc = dtype == SKDSP_C128 ? equalize_run<double, double>(rawz, p.ndata * nf, 1, pil, nullptr, p.npilot, p.ndata, nrow, nf, npb, z_dev, z_stride, s)
                                     : equalize_run<double, float>(rawz, p.ndata * nf, 1, pil, nullptr, p.npilot, p.ndata, nrow, nf, npb, z_dev, z_stride, s);
            if (rc) return rc;
        }
        note_path("ofdm_chanest");
    }
    return SKDSP_OK;
}

int ofdm_equalize_check(int64_t nsym, int64_t nrow, int dtype, int nf, int npb, int64_t z_stride, int64_t out_stride)
{
    SK_CHECK(dtype == SKDSP_C64 || dtype == SKDSP_C128, SKDSP_ERR_BADARG, "ofdm_equalize: complex64 or complex128 rows (dtype code %d)", dtype);
    SK_CHECK(nf >= 1 && nf <= (1 << psd::kMaxLog2) && npb >= 2, SKDSP_ERR_BADARG, "ofdm_equalize: need 1 <= nf <= 4096 and npb >= 2 (nf = %d, npb = %d)", nf, npb);
    SK_CHECK(nsym >= 0 && nrow >= 0 && nsym <= kMaxElems / (2 * nf), SKDSP_ERR_BADARG, "ofdm_equalize: %lld symbols in %lld rows", (long long)nsym, (long long)nrow);
    const int64_t ndata = nsym - ofdm::rx_pilots(nsym, npb);
    SK_CHECK(rows_fit(nsym * nf, z_stride, nrow) && rows_fit(ndata * nf, out_stride, nrow), SKDSP_ERR_BADARG, "ofdm_equalize: the rows overlap (strides %lld, %lld)",
             (long long)z_stride, (long long)out_stride);
    return SKDSP_OK;
}

// chan_est_equalize on the rows of a caller's z ([nsym, nf] each): the estimator, then the division of the data rows
int ofdm_equalize_launch(const void *z_dev, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht_host,
                         void *scratch_dev, void *out_dev, int64_t out_stride, void *h_dev, hipStream_t s)
{
    int rc = ofdm_equalize_check(nsym, nrow, dtype, nf, npb, z_stride, out_stride);
    if (rc) return rc;
    if (nrow == 0 || nsym == 0) return SKDSP_OK;
    const size_t esz = dtype_size(dtype);
    const int64_t npilot = ofdm::rx_pilots(nsym, npb), ndata = nsym - npilot;
    SK_CHECK(z_dev && scratch_dev && h_dev && (out_dev || ndata == 0), SKDSP_ERR_BADARG, "ofdm_equalize: null pointer");
    SK_CHECK((((uintptr_t)z_dev | (uintptr_t)out_dev) & (esz - 1)) == 0 && ((uintptr_t)h_dev & 15) == 0 && ((uintptr_t)scratch_dev & 255) == 0, SKDSP_ERR_BADARG,
             "ofdm_equalize: the pointers must be aligned to their elements");
    char *sc = static_cast<char *>(scratch_dev);
    cx<double> *hht = hht_host ? reinterpret_cast<cx<double> *>(sc) : nullptr;
    double *est = reinterpret_cast<double *>(sc + tab_bytes(nf));
    if (hht) SK_HIP(hipMemcpyAsync(hht, hht_host, (size_t)nf * 16, hipMemcpyHostToDevice, s));
    if (dtype == SKDSP_C128) {
        if ((rc = chanest_run<double>(z_dev, z_stride, (int64_t)npb * nf, npilot, nrow, nf, alpha, est, (double *)h_dev, s))) return rc;
        rc = equalize_run<double, double>(z_dev, z_stride, 0, est, hht, npilot, ndata, nrow, nf, npb, out_dev, out_stride, s);
    } else {
        if ((rc = chanest_run<float>(z_dev, z_stride, (int64_t)npb * nf, npilot, nrow, nf, alpha, est, (double *)h_dev, s))) return rc;
        rc = equalize_run<float, float>(z_dev, z_stride, 0, est, hht, npilot, ndata, nrow, nf, npb, out_dev, out_stride, s);
    }
    if (rc) return rc;
    note_path("ofdm_chanest");
    return SKDSP_OK;
}

}  // namespace skdsp
