// psd.hip -- the Welch primitive behind sigsys.psd / my_psd / simple_sa (sigsys.py:2497-2585, 2457-2494, 1008-1084).  gfx950.
//
//     S[k] = sum_{i < nseg} | sum_{n < ns} w[n] x[i step + n] exp(-2 pi j k n / n_fft) |^2,   k < n_fft, float64
//
// psd_kernel: a workgroup owns spw consecutive segments.  It walks them in chunks of cs segments whose input span is staged
// in an LDS ring addressed by the ABSOLUTE sample index modulo the ring size, so a sample two chunks share stays where it is
// and only the samples behind the previous chunk are loaded (16-byte nontemporal loads): within a workgroup every sample is
// fetched once, and neighbouring workgroups share ns - step samples.  Each round cuts NB segments (complex input) or
// 2 NB (real input: segments 2m and 2m+1 as the real and imaginary part of one transform) out of the ring, times the
// window, through the in-place FFT of psd_core.hpp (float64 butterflies; the LDS image is float64 too unless option
// psd_f32_image asks for float32), and adds |X|^2 per position to float64 registers -- the segment sum never passes through
// float32.  For the packed pair |A[k]|^2 + |B[k]|^2 = (|Z[k]|^2 + |Z[N-k]|^2) / 2, so nothing is
// untangled: the fold happens once, in the reduction.  At the end the workgroup sums its NB side-by-side copies in a fixed
// order and writes one row of n_fft float64 partial sums in bin order.
// psd_reduce_kernel: adds the rows in a fixed order (16 interleaved strands per bin, then the strands in order) and folds
// real input.  No atomics anywhere: the result is bit-identical from run to run.
//
// Every sample of a segment is multiplied by its window value and enters every bin through additions only, so one nan or
// inf in a used sample (also under w = 0) makes all bins non-finite; samples behind the last segment never reach a segment.
#include <math.h>
#include <string.h>
#include <algorithm>
#include "skdsp_internal.hpp"
#include "psd_core.hpp"

namespace skdsp {
namespace {

using psd::cx;
using psd::kThreads;

struct PsdArgs {
    int64_t n, nseg, step;
    int ns, spw, cs, cap;   // segments per workgroup / per chunk, ring size in samples
};

// SI: the signal's scalar type, T: the LDS image's; window, twiddles and butterflies are float64 (psd_core.hpp)
template <typename SI, typename T, int NC, int LOG2N>
__global__ __launch_bounds__(kThreads) void psd_kernel(const SI *__restrict__ x, PsdArgs a, const double *__restrict__ win,
                                                       const cx<double> *__restrict__ tw, double *__restrict__ partial)
{
    typedef psd::Core<T, double, LOG2N> C;
    constexpr int N = C::N, PACK = NC == 1 ? 2 : 1, ROUND = C::NB * PACK;
    constexpr int VE = 16 / (int)(sizeof(SI) * NC);   // samples per 16-byte load
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    cx<T> *work = reinterpret_cast<cx<T> *>(psd_smem);                             // NB images of N points
    SI *ring = reinterpret_cast<SI *>(psd_smem + sizeof(cx<T>) * C::NB * N);      // a.cap samples

    const int tid = threadIdx.x, sb = tid / C::TS, t = tid % C::TS;
    cx<T> *img = work + sb * N;
    double acc[C::NACC];
    SK_UNROLL
    for (int i = 0; i < C::NACC; ++i) acc[i] = 0.0;

    const int64_t seg0 = (int64_t)blockIdx.x * a.spw, segE = min(a.nseg, seg0 + a.spw);
    const bool x16 = ((uintptr_t)x & 15) == 0;
    int64_t loaded_end = seg0 * a.step;
    loaded_end -= loaded_end % VE;

    for (int64_t c0 = seg0; c0 < segE; c0 += a.cs) {
        const int64_t ce = min(segE, c0 + a.cs);
        const int64_t need_lo = c0 * a.step, need_hi = (ce - 1) * a.step + a.ns;
        const int64_t lo = max(loaded_end, need_lo - need_lo % VE), hi = need_hi + (VE - need_hi % VE) % VE;
        // (the previous chunk's last round ends with a barrier: its ring reads are done)
        if (hi > lo) {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const int nv = (int)((hi - lo) / VE), pos0 = (int)(lo % a.cap);
            for (int v = tid; v < nv; v += kThreads) {
                const int64_t i0 = lo + (int64_t)v * VE;
                int pos = pos0 + v * VE;
                if (pos >= a.cap) pos -= a.cap;
                SI *d = ring + pos * NC;
                if (x16 && i0 + VE <= a.n) {
                    *reinterpret_cast<v4u *>(d) = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(x + i0 * NC));
                } else {
                    SK_UNROLL
                    for (int e = 0; e < VE * NC; ++e) d[e] = (i0 + e / NC < a.n) ? x[i0 * NC + e] : SI(0);
                }
            }
            loaded_end = hi;
        }
        __syncthreads();
        const int cpos = (int)(need_lo % a.cap);
        for (int64_t r0 = c0; r0 < ce; r0 += ROUND) {
            const int64_t sA = r0 + sb * PACK;
            const bool active = sA < ce, second = PACK == 2 && sA + 1 < ce;
            int baseA = 0, baseB = 0;
            if (active) {
                baseA = cpos + (int)((sA - c0) * a.step);
                if (baseA >= a.cap) baseA -= a.cap;
            }
            if (second) {
                baseB = baseA + (int)a.step;
                if (baseB >= a.cap) baseB -= a.cap;
            }
            auto ld = [&](int n) -> cx<double> {
                if (!active || n >= a.ns) return cx<double>{0.0, 0.0};
                const double w = win[n];
                int p = baseA + n;
                if (p >= a.cap) p -= a.cap;
                if constexpr (NC == 2) {
                    return cx<double>{(double)ring[2 * p] * w, (double)ring[2 * p + 1] * w};
                } else {
                    double b = 0.0;
                    if (second) {
                        int q = baseB + n;
                        if (q >= a.cap) q -= a.cap;
                        b = (double)ring[q] * w;
                    }
                    return cx<double>{(double)ring[p] * w, b};
                }
            };
            C::first(t, ld, tw, img);
            __syncthreads();
            SK_UNROLL
            for (int s = 1; s < C::NSTORE; ++s) {
                C::mid(s, t, tw, img);
                __syncthreads();
            }
            if (active) C::last(t, img, acc);
            __syncthreads();
        }
    }

    // the NB side-by-side copies, in order, into one row in bin order
    double *red = reinterpret_cast<double *>(psd_smem);
    SK_UNROLL
    for (int i = 0; i < C::NACC; ++i) red[sb * N + C::bin_of(4 * (t + C::TS * (i >> 2)) + (i & 3))] = acc[i];
    __syncthreads();
    for (int f = tid; f < N; f += kThreads) {
        double s = red[f];
        for (int b = 1; b < C::NB; ++b) s += red[b * N + f];
        partial[(size_t)blockIdx.x * N + f] = s;
    }
}

// S[f] = sum over rows (fold: half of that for f plus that for n_fft - f).  16 bins x 16 strands per workgroup.
__global__ __launch_bounds__(256) void psd_reduce_kernel(const double *__restrict__ partial, int rows, int n_fft, int fold,
                                                         double *__restrict__ S)
{
    __shared__ double sh[2][16][16];
    const int j = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int f = blockIdx.x * 16 + j, f2 = (n_fft - f) & (n_fft - 1);
    double s = 0.0, s2 = 0.0;
    for (int r = g; r < rows; r += 16) s += partial[(size_t)r * n_fft + f];
    if (fold)
        for (int r = g; r < rows; r += 16) s2 += partial[(size_t)r * n_fft + f2];
    sh[0][g][j] = s;
    sh[1][g][j] = s2;
    __syncthreads();
    if (g == 0) {
        double a = sh[0][0][j], b = sh[1][0][j];
        for (int k = 1; k < 16; ++k) {
            a += sh[0][k][j];
            b += sh[1][k][j];
        }
        S[f] = fold ? 0.5 * (a + b) : a;
    }
}

// ---- host tables: the window and the twiddles exp(-2 pi j i / n_fft) in float64; kept per (device, n_fft, window)
struct PsdTab {
    int device, log2n;
    std::vector<double> win;
    DevTable<double> win_dev, tw_dev;   // tw: complex128, interleaved
};
std::mutex g_tab_mu;
// Most recently used first.  Never destroyed: the tables own device memory, and a free during static destruction -- after the runtime
// has torn down -- hangs or aborts the exit of the process; nothing device-side runs then.
std::vector<PsdTab> &g_tabs = *new std::vector<PsdTab>();
constexpr size_t kMaxTabs = 16;
constexpr int kMaxDevices = 64;

// LDS bytes a workgroup may ask for, read from the device once
static int lds_limit(int dev, int *out)
{
    static std::mutex mu;
    static int cached[kMaxDevices] = {};
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 0 && dev < kMaxDevices && cached[dev]) {
        *out = cached[dev];
        return SKDSP_OK;
    }
    int v = 0;
    SK_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (dev >= 0 && dev < kMaxDevices) cached[dev] = v;
    *out = v;
    return SKDSP_OK;
}

static int upload_tables(PsdTab &tb)
{
    const int N = 1 << tb.log2n;
    std::vector<cx<double>> tw(N);
    const double kTwoPi = 6.283185307179586476925286766559;
    for (int i = 0; i < N; ++i) tw[i] = cx<double>{cos(kTwoPi * i / N), -sin(kTwoPi * i / N)};
    const int rc = tb.win_dev.upload(tb.win);
    return rc ? rc : tb.tw_dev.upload(&tw[0].x, (size_t)2 * N);
}

static int tables_for(int log2n, const double *window, int ns, void **win_dev, void **tw_dev)
{
    std::lock_guard<std::mutex> lk(g_tab_mu);
    const int dev = ctx().device;
    // a repeated call finds its tables in front: one comparison of ns doubles (the window is the caller's host array, so
    // its values are the only key there is)
    for (size_t i = 0; i < g_tabs.size(); ++i) {
        PsdTab &tb = g_tabs[i];
        if (tb.device == dev && tb.log2n == log2n && (int)tb.win.size() == ns && memcmp(tb.win.data(), window, sizeof(double) * ns) == 0) {
            *win_dev = tb.win_dev.dev;
            *tw_dev = tb.tw_dev.dev;
            if (i) std::rotate(g_tabs.begin(), g_tabs.begin() + i, g_tabs.begin() + i + 1);
            return SKDSP_OK;
        }
    }
    if (g_tabs.size() >= kMaxTabs) g_tabs.pop_back();   // least recently used out (the free waits for the device)
    PsdTab tb;
    tb.device = dev;
    tb.log2n = log2n;
    tb.win.assign(window, window + ns);
    int rc = upload_tables(tb);
    if (rc) return rc;
    *win_dev = tb.win_dev.dev;
    *tw_dev = tb.tw_dev.dev;
    g_tabs.insert(g_tabs.begin(), std::move(tb));
    return SKDSP_OK;
}

template <typename SI, typename T, int NC, int LOG2N>
static int launch_one(const void *x, const PsdArgs &a, const void *win, const void *tw, double *partial, int rows, size_t lds,
                      hipStream_t s)
{
    auto kern = psd_kernel<SI, T, NC, LOG2N>;
    // the dynamic LDS limit of this instantiation, raised once per device to the largest size asked for so far
    static std::mutex mu;
    static size_t granted[kMaxDevices] = {};
    const int dev = ctx().device;
    if (lds > 48 * 1024) {
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= kMaxDevices || lds > granted[dev]) {
            SK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (dev >= 0 && dev < kMaxDevices) granted[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(kThreads), lds, s, (const SI *)x, a, (const double *)win,
                       (const cx<double> *)tw, partial);
    return SKDSP_OK;
}

template <typename SI, typename T, int NC, typename... A> static int launch_log2(int log2n, A... args)
{
    switch (log2n) {
    case 6: return launch_one<SI, T, NC, 6>(args...);
    case 7: return launch_one<SI, T, NC, 7>(args...);
    case 8: return launch_one<SI, T, NC, 8>(args...);
    case 9: return launch_one<SI, T, NC, 9>(args...);
    case 10: return launch_one<SI, T, NC, 10>(args...);
    case 11: return launch_one<SI, T, NC, 11>(args...);
    default: return launch_one<SI, T, NC, 12>(args...);
    }
}

}  // namespace

int psd_check(int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg)
{
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "psd: bad dtype %d", dtype);
    SK_CHECK(n_fft >= (1 << psd::kMinLog2) && n_fft <= (1 << psd::kMaxLog2) && (n_fft & (n_fft - 1)) == 0, SKDSP_ERR_BADARG,
             "psd: n_fft must be a power of two in 64 ... 4096 (got %d)", n_fft);
    SK_CHECK(ns >= 1 && ns <= n_fft, SKDSP_ERR_BADARG, "psd: window length %d outside 1 ... n_fft = %d", ns, n_fft);
    SK_CHECK(step >= 1 && nseg >= 1, SKDSP_ERR_BADARG, "psd: step %lld and segment count %lld must be positive", (long long)step,
             (long long)nseg);
    SK_CHECK(n >= ns && (nseg - 1) <= (n - ns) / step, SKDSP_ERR_BADARG,
             "psd: %lld segments of %d samples, %lld apart, do not fit %lld samples", (long long)nseg, ns, (long long)step, (long long)n);
    SK_CHECK(window, SKDSP_ERR_BADARG, "psd: null window");
    return SKDSP_OK;
}

int psd_launch(const void *x, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg,
               double *S, hipStream_t s)
{
    int rc = psd_check(n, dtype, window, ns, n_fft, step, nseg);
    if (rc) return rc;
    SK_CHECK(x && S, SKDSP_ERR_BADARG, "psd: null pointer");
    int log2n = 0;
    while ((1 << log2n) < n_fft) ++log2n;
    const bool dbl = dtype_double(dtype), cplx = dtype_complex(dtype);
    const int sbytes = (int)dtype_size(dtype), ve = 16 / sbytes;
    const int nb = std::max(1, 1024 / n_fft), round = nb * (cplx ? 1 : 2);

    // LDS: the NB images, then the ring.  32 KiB of ring unless one round's span needs more; never less than one segment.
    int lds_max = 0;
    if ((rc = lds_limit(ctx().device, &lds_max))) return rc;
    lds_max = std::min(lds_max, 160 * 1024);
    const bool img64 = dbl || !opt().psd_f32_image;   // the LDS image's scalar type (psd_core.hpp: why float64 for float32 signals too)
    const int64_t work = (int64_t)nb * n_fft * 2 * (img64 ? 8 : 4);
    const int64_t ring_min = (int64_t)((ns + ve - 1) / ve * ve + 2 * ve) * sbytes;
    const int64_t ring_round = ((int64_t)(round - 1) * std::min<int64_t>(step, 1 << 20) + ns + 2 * ve) * sbytes;
    int64_t ring = std::max<int64_t>(32 * 1024, ring_round);
    ring = std::min(ring, (int64_t)lds_max - work);
    SK_CHECK(ring >= ring_min, SKDSP_ERR_BADARG, "psd: n_fft %d does not fit the %d bytes of LDS", n_fft, lds_max);
    int cap = (int)(ring / sbytes);
    cap -= cap % ve;
    SK_CHECK(cap >= ns + 2 * ve, SKDSP_ERR_UNSUPPORTED, "psd: ring of %d samples for a window of %d", cap, ns);
    int64_t cs = ((int64_t)cap - 2 * ve - ns) / step + 1;
    if (cs > round) cs -= cs % round;
    else if (!cplx && cs > 1) cs -= cs & 1;   // real input: segments pair within a chunk, so an odd chunk would end on a half-empty transform
    cs = std::min<int64_t>(cs, 1 << 16);

    const int rows_target = n_fft <= 1024 ? 1024 : 512;
    int64_t spw = (nseg + rows_target - 1) / rows_target;
    spw = (spw + cs - 1) / cs * cs;
    SK_CHECK(spw < ((int64_t)1 << 30), SKDSP_ERR_BADARG, "psd: %lld segments in one launch", (long long)nseg);
    const int rows = (int)((nseg + spw - 1) / spw);

    void *win_dev = nullptr, *tw_dev = nullptr, *partial = nullptr;
    if ((rc = tables_for(log2n, window, ns, &win_dev, &tw_dev))) return rc;
    if ((rc = ws_reserve(3, (size_t)rows * n_fft * sizeof(double) + 256, &partial))) return rc;

    PsdArgs a{n, nseg, step, ns, (int)spw, (int)cs, cap};
    const size_t lds = (size_t)work + (size_t)cap * sbytes;
    double *pd = (double *)partial;
    switch (dtype) {
    case SKDSP_F32:
        rc = img64 ? launch_log2<float, double, 1>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s)
                   : launch_log2<float, float, 1>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s);
        break;
    case SKDSP_C64:
        rc = img64 ? launch_log2<float, double, 2>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s)
                   : launch_log2<float, float, 2>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s);
        break;
    case SKDSP_F64: rc = launch_log2<double, double, 1>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s); break;
    default:        rc = launch_log2<double, double, 2>(log2n, x, a, win_dev, tw_dev, pd, rows, lds, s); break;
    }
    if (rc) return rc;
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(psd_reduce_kernel, dim3((unsigned)(n_fft / 16)), dim3(256), 0, s, (const double *)pd, rows, n_fft,
                       cplx ? 0 : 1, S);
    SK_HIP(hipGetLastError());
    note_path("psd");
    return SKDSP_OK;
}

}  // namespace skdsp
