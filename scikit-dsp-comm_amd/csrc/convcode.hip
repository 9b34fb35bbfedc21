// convcode.hip -- the FEC chain around the Viterbi decoder on the device: fec_conv.FECConv.conv_encoder, puncture and depuncture
// (fec_conv.py:501-712 of the reference) over the rows of a frame set, and the count of differing bits behind digitalcom.bit_errors
// (digitalcom.py:353-415).  gfx950.  The plans, the staging and the per-item functions are convcode_core.hpp, shared with
// tests/host/convcode_emul.cpp.
//
//   convenc_kernel<R>      work item = (row, run of 4096 bits), dealt over the whole grid: one row of 2^26 bits fills the device like 4096
//                          rows of 16384.  The item's window (its bits and the K - 1 bytes before them) is staged into LDS in aligned 16-byte
//                          chunks, a lane forms the word of its 16 bits and the K - 1 before them, each polynomial's 16 outputs are the XOR of
//                          the shifts its mask selects, and the R * 4096 output bytes leave from a second image in aligned 16-byte chunks.
//   puncture_kernel<T>, depuncture_kernel<T>
//                          one periodic gather (output o = q P_out + r reads input q P_in + tab[r] or takes the erase value) over elements
//                          of 1, 2, 4 or 8 bytes; the period table comes from the host and sits in LDS.
//   bitcount_kernel        work item = (row, 4096 bytes): both streams staged at their own alignment, 16 bytes per lane, the item's sum added
//                          to the row's int64 with an integer atomic (order-independent: identical from run to run).
// Nothing outside a row's [start, end) is read or written, whatever the pointers' alignment.  No scratch.
#include <memory>
#include "skdsp_internal.hpp"
#include "convcode_core.hpp"

namespace skdsp {
namespace {

struct DevMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *g) const { return *g; }
    __device__ __forceinline__ void st8(uint8_t *g, uint8_t v) const { *g = v; }
    __device__ __forceinline__ void in16(uint8_t *img, const uint8_t *g) const { *reinterpret_cast<uint4 *>(img) = *reinterpret_cast<const uint4 *>(g); }
    __device__ __forceinline__ void out16(uint8_t *g, const uint8_t *img) const { *reinterpret_cast<uint4 *>(g) = *reinterpret_cast<const uint4 *>(img); }
};

struct DevElem {
    template <typename T> __device__ __forceinline__ T ld(const T *g) const { return *g; }
    template <typename T> __device__ __forceinline__ void st(T *g, T v) const { *g = v; }
};

// ------------------------------------------------------------------------------------------------------------------ encoder
struct EncArgs {
    const uint8_t *bits;
    uint8_t *code;
    const uint8_t *states_in;   // null: rest
    uint8_t *states_out;        // null: not wanted
    int64_t n;
    uint32_t items;             // per row
    int per_row_state;          // states_in holds one state per row (else one for all)
    cvc::EncPlan plan;
};

template <int R> __global__ __launch_bounds__(cvc::kThreads) void convenc_kernel(EncArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t img_in[cvc::kEncInBytes];
    __shared__ __attribute__((aligned(16))) uint8_t img_out[blk::image_bytes(R * cvc::kEncWg)];
    cvc::EncPlan p = a.plan;
    p.R = R;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int len = cvc::enc_len(a.n, it), h = cvc::enc_hist(p, it);
    const uint8_t *gin = a.bits + row * a.n + cvc::enc_first(it) - h;
    uint8_t *gout = a.code + (row * a.n + cvc::enc_first(it)) * R;
    const DevMem mem;
    blk::stage_in(mem, gin, h + len, img_in, t, cvc::kThreads);
    __syncthreads();
    const int i0 = cvc::kEncRun * t;
    if (i0 < len) {
        uint32_t state = 0;
        if (it == 0 && t == 0 && a.states_in) state = a.states_in[a.per_row_state ? row : 0] & ((1u << (p.K - 1)) - 1u);
        const uint32_t w = cvc::enc_lane_word(p, img_in, blk::lead_of(gin), h, len, i0, state);
        const int cnt = len - i0 < cvc::kEncRun ? len - i0 : cvc::kEncRun;
        cvc::enc_put(p, w, cnt, img_out + blk::lead_of(gout) + R * i0);
        if (a.states_out && i0 + cnt == len && it + 1 == a.items) a.states_out[row] = (uint8_t)cvc::enc_state_after(p, w, cnt - 1);
    }
    __syncthreads();
    blk::stage_out(mem, gout, R * len, img_out, t, cvc::kThreads);
}

// ------------------------------------------------------------------------------------------------------------------ puncture / depuncture
struct GatherArgs {
    const void *x;
    void *y;
    int64_t n_in, n_out;        // elements per input / output row
    uint32_t items;             // per row
    int p_in, p_out;
    uint64_t erase;             // the erase value's bytes
    uint32_t tab[2 * cvc::kMaxPattern / 4];
};

template <typename T> __device__ __forceinline__ void gather_item(const GatherArgs &a)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab32[2 * cvc::kMaxPattern / 4];
    const int t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 2 * cvc::kMaxPattern / 4; ++i) tab32[i] = a.tab[i];   // (constant indices: scalar loads of the arguments)
    }
    __syncthreads();
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(tab32);
    const int64_t row = blockIdx.x / a.items;
    const uint32_t it = blockIdx.x - (uint32_t)row * a.items;   // (the difference fits: it < items)
    const T *x = static_cast<const T *>(a.x) + row * a.n_in;
    T *y = static_cast<T *>(a.y) + row * a.n_out;
    cvc::gather_thread<T>(DevElem(), tab, a.p_in, a.p_out, x, y, a.n_out, (T)a.erase, it, t);
}
template <typename T> __global__ __launch_bounds__(cvc::kThreads) void puncture_kernel(GatherArgs a) { gather_item<T>(a); }
template <typename T> __global__ __launch_bounds__(cvc::kThreads) void depuncture_kernel(GatherArgs a) { gather_item<T>(a); }

// ------------------------------------------------------------------------------------------------------------------ count
struct CntArgs {
    const uint8_t *tx, *rx;
    int64_t tx_stride, rx_stride, n;
    uint32_t items;
    int invert;
    unsigned long long *counts;
};

__global__ __launch_bounds__(cvc::kThreads) void bitcount_kernel(CntArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t img_t[cvc::kCntImgBytes];
    __shared__ __attribute__((aligned(16))) uint8_t img_r[cvc::kCntImgBytes];
    __shared__ int red[cvc::kThreads / 64];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.items, it = blockIdx.x - row * a.items;
    const int64_t first = it * cvc::kCntWg;
    const int len = a.n - first < cvc::kCntWg ? (int)(a.n - first) : cvc::kCntWg;
    const uint8_t *gt = a.tx + row * a.tx_stride + first, *gr = a.rx + row * a.rx_stride + first;
    const DevMem mem;
    blk::stage_in(mem, gt, len, img_t, t, cvc::kThreads);
    blk::stage_in(mem, gr, len, img_r, t, cvc::kThreads);
    __syncthreads();
    int c = cvc::cnt_lane(img_t, blk::lead_of(gt), img_r, blk::lead_of(gr), len, 16 * t, a.invert);
    for (int off = 1; off < 64; off <<= 1) c += __shfl_xor(c, off);
    if ((t & 63) == 0) red[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int v = 0; v < cvc::kThreads / 64; ++v) s += red[v];
        if (s) atomicAdd(a.counts + row, (unsigned long long)s);
    }
}

struct ConvHandle : HandleBase {
    cvc::EncPlan plan;
};

bool grid_fits(int64_t items, int64_t nrow) { return items == 0 || nrow <= (((int64_t)1 << 31) - 1) / items; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host side
// argument errors need no device, and neither does the handle: the masks travel as kernel arguments
int convcode_create(const char *const *polys, int npoly, HandleBase **out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "convcode_create: null out");
    cvc::EncPlan plan;
    const char *why = cvc::enc_plan_make(polys, npoly, &plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "convcode_create: %s", why);
    std::unique_ptr<ConvHandle> h(new ConvHandle());
    h->kind = H_CONVCODE;
    h->dtype = 0;
    h->plan = plan;
    *out = h.release();
    return SKDSP_OK;
}

void convcode_sizes(HandleBase *hb, int *K, int *R)
{
    ConvHandle *h = static_cast<ConvHandle *>(hb);
    *K = h->plan.K;
    *R = h->plan.R;
}

int convcode_check(HandleBase *, int64_t n, int64_t nrow, int64_t nstates_in)
{
    SK_CHECK(n >= 0 && nrow >= 0, SKDSP_ERR_BADARG, "convcode: negative size (n = %lld, nrow = %lld)", (long long)n, (long long)nrow);
    SK_CHECK(nstates_in == 0 || nstates_in == 1 || nstates_in == nrow, SKDSP_ERR_BADARG, "convcode: 0, 1 or nrow initial states (got %lld for %lld rows)",
             (long long)nstates_in, (long long)nrow);
    SK_CHECK(n < ((int64_t)1 << 40) && grid_fits(cvc::enc_items_per_row(n), nrow), SKDSP_ERR_BADARG, "convcode: %lld rows of %lld bits in one launch",
             (long long)nrow, (long long)n);
    return SKDSP_OK;
}

// nrow rows of n bytes 0 / 1 -> nrow rows of R n bytes; states: one byte per row, the state string read as a binary number
int convcode_launch(HandleBase *hb, const uint8_t *bits_dev, int64_t n, int64_t nrow, const uint8_t *states_in_dev, int64_t nstates_in, uint8_t *code_dev,
                    uint8_t *states_out_dev, hipStream_t s)
{
    ConvHandle *h = static_cast<ConvHandle *>(hb);
    int rc = convcode_check(hb, n, nrow, nstates_in);
    if (rc) return rc;
    SK_CHECK(nstates_in == 0 || states_in_dev, SKDSP_ERR_BADARG, "convcode: null initial states");
    if (nrow == 0) return SKDSP_OK;
    if (n == 0) {   // nothing to encode: the states pass through, no launch
        if (!states_out_dev) return SKDSP_OK;
        if (nstates_in == 0) SK_HIP(hipMemsetAsync(states_out_dev, 0, (size_t)nrow, s));
        else if (nstates_in == nrow) SK_HIP(hipMemcpyAsync(states_out_dev, states_in_dev, (size_t)nrow, hipMemcpyDeviceToDevice, s));
        else
            for (int64_t r = 0; r < nrow; ++r) SK_HIP(hipMemcpyAsync(states_out_dev + r, states_in_dev, 1, hipMemcpyDeviceToDevice, s));
        return SKDSP_OK;
    }
    SK_CHECK(bits_dev && code_dev, SKDSP_ERR_BADARG, "convcode: null pointer");
    EncArgs a;
    a.bits = bits_dev;
    a.code = code_dev;
    a.states_in = nstates_in ? states_in_dev : nullptr;
    a.states_out = states_out_dev;
    a.n = n;
    a.items = (uint32_t)cvc::enc_items_per_row(n);
    a.per_row_state = nstates_in == nrow && nrow > 1;
    a.plan = h->plan;
    const unsigned grid = (unsigned)(a.items * nrow);
    if (h->plan.R == 2) hipLaunchKernelGGL(convenc_kernel<2>, dim3(grid), dim3(cvc::kThreads), 0, s, a);
    else hipLaunchKernelGGL(convenc_kernel<3>, dim3(grid), dim3(cvc::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("convenc");
    return SKDSP_OK;
}

int gather_check(int depuncture, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out)
{
    const char *name = depuncture ? "depuncture" : "puncture";
    SK_CHECK(n >= 0 && nrow >= 0 && n < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "%s: rows of 0 ... 2^31 - 1 elements (n = %lld, nrow = %lld)", name, (long long)n,
             (long long)nrow);
    SK_CHECK(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, SKDSP_ERR_BADARG, "%s: elements of 1, 2, 4 or 8 bytes (got %d)", name, elem_bytes);
    const char *why = cvc::pattern_check(mask1, mask2, L_pp);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "%s: %s", name, why);
    const int64_t len = depuncture ? cvc::depuncture_out_len(n, mask1, L_pp) : cvc::puncture_out_len(n, mask1, L_pp);
    SK_CHECK(len < ((int64_t)1 << 31) && grid_fits(cvc::gather_items_per_row(len), nrow), SKDSP_ERR_BADARG, "%s: %lld rows of %lld elements in one launch", name,
             (long long)nrow, (long long)len);
    if (n_out) *n_out = len;
    return SKDSP_OK;
}

template <typename T> static void gather_go(int depuncture, const GatherArgs &a, unsigned grid, hipStream_t s)
{
    if (depuncture) hipLaunchKernelGGL(depuncture_kernel<T>, dim3(grid), dim3(cvc::kThreads), 0, s, a);
    else hipLaunchKernelGGL(puncture_kernel<T>, dim3(grid), dim3(cvc::kThreads), 0, s, a);
}

// nrow rows of n elements -> nrow rows of the out_len elements; erase: the element's bytes (depuncture only)
int gather_launch(int depuncture, const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase,
                  void *y_dev, hipStream_t s)
{
    int64_t n_out = 0;
    int rc = gather_check(depuncture, n, nrow, elem_bytes, mask1, mask2, L_pp, &n_out);
    if (rc) return rc;
    SK_CHECK(!depuncture || erase, SKDSP_ERR_BADARG, "depuncture: null erase value");
    if (nrow == 0 || n_out == 0) return SKDSP_OK;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "%s: null pointer", depuncture ? "depuncture" : "puncture");
    SK_CHECK(elem_aligned(x_dev, y_dev, elem_bytes), SKDSP_ERR_BADARG, "%s: the pointers must be aligned to the element", depuncture ? "depuncture" : "puncture");
    cvc::GatherPlan g;
    cvc::gather_plan_make(mask1, mask2, L_pp, depuncture != 0, &g);
    GatherArgs a;
    a.x = x_dev;
    a.y = y_dev;
    a.n_in = n;
    a.n_out = n_out;
    a.items = (uint32_t)cvc::gather_items_per_row(n_out);
    a.p_in = g.p_in;
    a.p_out = g.p_out;
    a.erase = 0;
    if (depuncture) memcpy(&a.erase, erase, (size_t)elem_bytes);
    memcpy(a.tab, g.tab, sizeof(a.tab));
    const unsigned grid = (unsigned)(a.items * nrow);
    switch (elem_bytes) {
    case 1: gather_go<uint8_t>(depuncture, a, grid, s); break;
    case 2: gather_go<uint16_t>(depuncture, a, grid, s); break;
    case 4: gather_go<uint32_t>(depuncture, a, grid, s); break;
    default: gather_go<uint64_t>(depuncture, a, grid, s); break;
    }
    SK_HIP(hipGetLastError());
    note_path(depuncture ? "depuncture" : "puncture");
    return SKDSP_OK;
}

int bitcount_check(int64_t tx_stride, int64_t rx_stride, int64_t n, int64_t nrow)
{
    SK_CHECK(n >= 0 && nrow >= 0 && tx_stride >= 0 && rx_stride >= 0, SKDSP_ERR_BADARG, "bit_count: negative size or stride (n = %lld, nrow = %lld)", (long long)n,
             (long long)nrow);
    SK_CHECK(n < ((int64_t)1 << 40) && grid_fits(cvc::cnt_items_per_row(n), nrow), SKDSP_ERR_BADARG, "bit_count: %lld rows of %lld bytes in one launch", (long long)nrow,
             (long long)n);
    return SKDSP_OK;
}

// counts_dev[r] = the number of i < n with tx[r tx_stride + i] != rx[r rx_stride + i] (invert: with ==), int64
int bitcount_launch(const uint8_t *tx_dev, int64_t tx_stride, const uint8_t *rx_dev, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts_dev,
                    hipStream_t s)
{
    int rc = bitcount_check(tx_stride, rx_stride, n, nrow);
    if (rc) return rc;
    if (nrow == 0) return SKDSP_OK;
    SK_CHECK(counts_dev && ((uintptr_t)counts_dev & 7) == 0, SKDSP_ERR_BADARG, "bit_count: the counts must be an 8-byte aligned pointer");
    SK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)nrow * sizeof(int64_t), s));
    if (n == 0) return SKDSP_OK;
    SK_CHECK(tx_dev && rx_dev, SKDSP_ERR_BADARG, "bit_count: null pointer");
    CntArgs a;
    a.tx = tx_dev;
    a.rx = rx_dev;
    a.tx_stride = tx_stride;
    a.rx_stride = rx_stride;
    a.n = n;
    a.items = (uint32_t)cvc::cnt_items_per_row(n);
    a.invert = invert ? 1 : 0;
    a.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    hipLaunchKernelGGL(bitcount_kernel, dim3((unsigned)(a.items * nrow)), dim3(cvc::kThreads), 0, s, a);
    SK_HIP(hipGetLastError());
    note_path("bitcount");
    return SKDSP_OK;
}

}  // namespace skdsp
