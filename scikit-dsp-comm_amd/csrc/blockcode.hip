// blockcode.hip -- the block-code kernels behind fec_block.FECHamming.hamm_encoder / hamm_decoder and FECCyclic.cyclic_encoder /
// cyclic_decoder (fec_block.py:151-235, 292-423).  gfx950.
//
// Every code word is independent: a call is ONE launch over all its blocks, a byte stream in and a byte stream out.  The code is three
// tables of j-bit words built on the host (blockcode_core.hpp: the table form, the plan, the run staging and the per-block functions,
// shared with tests/host/blockcode_emul.cpp).  A workgroup
//   1. stages its run -- the contiguous input bytes of its blocks -- into an LDS image in aligned 16-byte chunks (partial chunks at the
//      run's two ends byte by byte), and, for the lane and wave forms, the tables into LDS;
//   2. forms each block's word and writes the block's output bytes into a second image laid out by the OUTPUT run's alignment:
//        lane form   one lane per block walks its n bytes (byte stride n, odd);
//        wave form   one wave per block, lanes take dwords, xor butterfly across the wave, then the wave writes the block's bytes;
//        group form  the whole workgroup on one block, wave words combined through LDS, tables through L2;
//   3. stores the output run in aligned 16-byte chunks.
// Nothing outside [in, in + nblocks * bytes_in) is read and nothing outside [out, out + nblocks * bytes_out) is written, whatever the
// two pointers' alignment.  No atomics, one launch per call: bit-identical from run to run.
#include <memory>
#include <mutex>
#include "skdsp_internal.hpp"
#include "blockcode_core.hpp"

namespace skdsp {
namespace {

struct BlkArgs {
    const uint8_t *in;
    uint8_t *out;
    const uint32_t *tab;    // enc (encode) or syn (decode), natural order
    const uint32_t *trap;   // decode only
    int64_t nblocks;
    blk::Plan plan;
};

struct DevMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *g) const { return *g; }
    __device__ __forceinline__ void st8(uint8_t *g, uint8_t v) const { *g = v; }
    __device__ __forceinline__ void in16(uint8_t *img, const uint8_t *g) const { *reinterpret_cast<uint4 *>(img) = *reinterpret_cast<const uint4 *>(g); }
    __device__ __forceinline__ void out16(uint8_t *g, const uint8_t *img) const { *reinterpret_cast<uint4 *>(g) = *reinterpret_cast<const uint4 *>(img); }
};

template <int FORM, int MODE, int THREADS>
__global__ __launch_bounds__(THREADS) void blockcode_kernel(BlkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t blk_smem[];
    blk::Plan p = a.plan;
    p.form = FORM;   // (what the launcher chose: a constant here)
    const int t = threadIdx.x, lane = t & (blk::kLanes - 1), wave = t / blk::kLanes;
    const int nin = blk::bytes_in(p, MODE), nout = blk::bytes_out(p, MODE);
    const int nb = blk::blocks_of(p, a.nblocks, blockIdx.x);
    const int64_t first = (int64_t)blockIdx.x * p.blocks_per_wg;
    const uint8_t *gin = a.in + first * nin;
    uint8_t *gout = a.out + first * nout;
    uint8_t *img_in = blk_smem + p.off_in, *img_out = blk_smem + p.off_out;
    uint32_t *tab_lds = reinterpret_cast<uint32_t *>(blk_smem + p.off_tab), *trap_lds = reinterpret_cast<uint32_t *>(blk_smem + p.off_trap);
    uint32_t *red = reinterpret_cast<uint32_t *>(blk_smem + p.off_red);
    const DevMem mem;

    blk::stage_in(mem, gin, nb * nin, img_in, t, THREADS);
    if (FORM != blk::kGroup) {
        for (int i = t; i < nin; i += THREADS) tab_lds[blk::tab_index(p, i)] = a.tab[i];
        if (MODE == blk::kDecode)
            for (int i = t; i < p.k; i += THREADS) trap_lds[i] = a.trap[i];
    }
    __syncthreads();

    const int s0 = blk::lead_of(gin), o0 = blk::lead_of(gout);
    if (FORM == blk::kLane) {
        if (t < nb) {
            const int s = s0 + t * nin, o = o0 + t * nout;
            const uint32_t w = blk::syndrome_word(p, img_in, s, nin, tab_lds, 0, 1);
            for (int i = 0; i < nout; ++i)
                img_out[o + i] = blk::emit(p, MODE, i, i < p.k ? img_in[s + i] : (uint8_t)0, w, MODE == blk::kDecode ? trap_lds[i] : 0u);
        }
    } else if (FORM == blk::kWave) {
        for (int b = wave; b < nb; b += THREADS / blk::kLanes) {
            const int s = s0 + b * nin, o = o0 + b * nout;
            uint32_t w = blk::syndrome_word(p, img_in, s, nin, tab_lds, lane, blk::kLanes);
            for (int off = 1; off < blk::kLanes; off <<= 1) w ^= __shfl_xor(w, off);
            for (int i = lane; i < nout; i += blk::kLanes)
                img_out[o + i] = blk::emit(p, MODE, i, i < p.k ? img_in[s + i] : (uint8_t)0, w, MODE == blk::kDecode ? trap_lds[i] : 0u);
        }
    } else {
        uint32_t w = blk::syndrome_word(p, img_in, s0, nin, a.tab, t, THREADS);
        for (int off = 1; off < blk::kLanes; off <<= 1) w ^= __shfl_xor(w, off);
        if (lane == 0) red[wave] = w;
        __syncthreads();
        w = 0;
        for (int v = 0; v < THREADS / blk::kLanes; ++v) w ^= red[v];
        for (int i = t; i < nout; i += THREADS)
            img_out[o0 + i] = blk::emit(p, MODE, i, i < p.k ? img_in[s0 + i] : (uint8_t)0, w, MODE == blk::kDecode ? a.trap[i] : 0u);
    }
    __syncthreads();
    blk::stage_out(mem, gout, nb * nout, img_out, t, THREADS);
}

struct BlkHandle : HandleBase {
    blk::Plan plan;
    DevTable<uint32_t> enc, syn, trap;
};

constexpr int kMaxDevices = 16;

template <int FORM, int MODE, int THREADS> static int launch_mode(const blk::Plan &plan, const BlkArgs &a, unsigned grid, hipStream_t s)
{
    auto kern = blockcode_kernel<FORM, MODE, THREADS>;
    const size_t lds = (size_t)plan.lds_bytes;
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
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), lds, s, a);
    return SKDSP_OK;
}
template <int FORM, int THREADS> static int launch_form(const blk::Plan &plan, int mode, const BlkArgs &a, unsigned grid, hipStream_t s)
{
    return mode == blk::kEncode ? launch_mode<FORM, blk::kEncode, THREADS>(plan, a, grid, s) : launch_mode<FORM, blk::kDecode, THREADS>(plan, a, grid, s);
}

}  // namespace

// argument errors need no device
int blockcode_create(int n, int k, const uint32_t *enc, const uint32_t *syn, const uint32_t *trap, HandleBase **out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "blockcode_create: null out");
    SK_CHECK(n >= 1 && k >= 1 && n <= 65535, SKDSP_ERR_BADARG, "blockcode_create: need 1 <= k < n <= 65535 (got n = %d, k = %d)", n, k);
    blk::Plan plan;
    const char *why = blk::plan_make(n, k, &plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "blockcode_create: %s (got n = %d, k = %d)", why, n, k);
    SK_CHECK(enc && syn && trap, SKDSP_ERR_BADARG, "blockcode_create: null table");
    SK_CHECK(blk::tables_fit(plan, enc, syn, trap), SKDSP_ERR_BADARG, "blockcode_create: a table word does not fit the %d parity bits", plan.j);
    {
        int rc = ensure_init();
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> ctxlk(ctx().mu);
    std::unique_ptr<BlkHandle> h(new BlkHandle());
    h->kind = H_BLOCKCODE;
    h->dtype = 0;
    h->plan = plan;
    int rc;
    if ((rc = h->enc.upload(enc, (size_t)k)) || (rc = h->syn.upload(syn, (size_t)n)) || (rc = h->trap.upload(trap, (size_t)k))) return rc;
    *out = h.release();
    return SKDSP_OK;
}

void blockcode_sizes(HandleBase *hb, int *n, int *k)
{
    BlkHandle *h = static_cast<BlkHandle *>(hb);
    *n = h->plan.n;
    *k = h->plan.k;
}

int blockcode_check(HandleBase *hb, int64_t nblocks)
{
    BlkHandle *h = static_cast<BlkHandle *>(hb);
    SK_CHECK(nblocks >= 0, SKDSP_ERR_BADARG, "blockcode: a negative number of blocks (%lld)", (long long)nblocks);
    SK_CHECK(blk::grid_of(h->plan, nblocks) < ((int64_t)1 << 31) && nblocks < ((int64_t)1 << 40), SKDSP_ERR_BADARG, "blockcode: %lld blocks in one launch", (long long)nblocks);
    return SKDSP_OK;
}

// mode 0: nblocks * k bytes (0 / 1) -> nblocks * n bytes; mode 1: the reverse.  Any byte alignment of either pointer.
int blockcode_launch(HandleBase *hb, int mode, const uint8_t *in_dev, int64_t nblocks, uint8_t *out_dev, hipStream_t s)
{
    BlkHandle *h = static_cast<BlkHandle *>(hb);
    int rc = blockcode_check(hb, nblocks);
    if (rc) return rc;
    if (nblocks == 0) return SKDSP_OK;
    SK_CHECK(in_dev && out_dev, SKDSP_ERR_BADARG, "blockcode: null pointer");
    BlkArgs a;
    a.in = in_dev;
    a.out = out_dev;
    a.tab = mode == blk::kEncode ? h->enc.dev : h->syn.dev;
    a.trap = h->trap.dev;
    a.nblocks = nblocks;
    a.plan = h->plan;
    const unsigned grid = (unsigned)blk::grid_of(h->plan, nblocks);
    switch (h->plan.form) {
    case blk::kLane: rc = launch_form<blk::kLane, 256>(h->plan, mode, a, grid, s); break;
    case blk::kWave: rc = launch_form<blk::kWave, 256>(h->plan, mode, a, grid, s); break;
    default: rc = launch_form<blk::kGroup, 1024>(h->plan, mode, a, grid, s); break;
    }
    if (rc) return rc;
    SK_HIP(hipGetLastError());
    note_path("blockcode");
    return SKDSP_OK;
}

}  // namespace skdsp
