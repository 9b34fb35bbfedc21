// viterbi.hip -- the register-exchange Viterbi decoder behind fec_conv.FECConv.viterbi_decoder (fec_conv.py:252-499).  gfx950.
//
// One lane per trellis state (viterbi_core.hpp: the trellis, the metrics, the per-state step and why the normalised int32 metrics
// decide exactly as the reference's float64 sums do).  A workgroup is ONE wave:
//   K <= 7 (Ns <= 64 states): 64 / Ns independent streams (rows) share the wave, lane = stream * Ns + state;
//   K = 8, 9 (Ns = 128, 256): one stream per wave, lane l holds states l, l + 64, ...; states m and m + Ns / 2 share their two
//   predecessors, which are fetched once per pair.
// Per step a stream broadcasts the symbol's 2 or 3 received values out of registers (a block of symbols is loaded one symbol per lane,
// the next block while this one is walked), forms each value's distance to code bit 0 and 1 once, picks its two branch metrics by its
// branch words, pulls the two predecessors' metrics and histories across lanes, keeps the survivor, and the stream's minimum (an xor
// butterfly that never leaves the stream's lanes), the first lane attaining it (ballot, find-first) and that lane's oldest history bit
// (a second ballot) give the decided bit.  64 decided bits leave as one burst of bytes.
// A call on a handle's own state (the reference object carries its trellis from call to call) reads and writes Ns metrics and histories
// in a small device buffer; the rows form starts every row from rest.  One launch per call, no atomics: bit-identical from run to run.
#include <string.h>
#include <memory>
#include "skdsp_internal.hpp"
#include "viterbi_core.hpp"

namespace skdsp {
namespace {

struct VitArgs {
    const void *x;        // nrow rows of nval values, x_stride values apart
    uint8_t *y;           // nrow rows of nout bytes (0 / 1), y_stride apart
    void *state;          // null: from rest, nothing kept (rows); else the handle's carried state (one row)
    int64_t nval, nsym, nout, nrow, x_stride, y_stride;
    int depth, R, top;
    uint32_t gmask[3];
};

template <int METRIC> struct XOf;
template <> struct XOf<vit::kHard> { typedef int8_t XT; typedef int VT; };
template <> struct XOf<vit::kSoft> { typedef int16_t XT; typedef int VT; };
template <> struct XOf<vit::kUnquant> { typedef double XT; typedef double VT; };

template <int METRIC, int K, int W>
__global__ __launch_bounds__(vit::kWave) void viterbi_kernel(VitArgs a)
{
    typedef typename XOf<METRIC>::XT XT;
    typedef typename XOf<METRIC>::VT VT;
    typedef typename vit::Dist<METRIC>::MT MT;
    constexpr int Ns = 1 << (K - 1), GL = vit::lanes_of(K), G = vit::kWave / GL, Q = vit::loads_of(K), B = GL * Q;
    constexpr int SPL = Ns > vit::kWave ? Ns / vit::kWave : 1, NP = SPL > 1 ? SPL / 2 : 1;
    const VT pad = METRIC == vit::kHard ? (VT)vit::kAbsent : (VT)0;

    const int lane = threadIdx.x, sub = lane % GL, base = lane - sub;
    const int64_t row = (int64_t)blockIdx.x * G + lane / GL;
    const bool active = row < a.nrow;
    const XT *x = static_cast<const XT *>(a.x) + (active ? row * a.x_stride : 0);
    uint8_t *y = a.y + (active ? row * a.y_stride : 0);
    const int R = a.R, depth = a.depth;

    // this lane's states: their branch words (even / odd predecessor) and input bits
    unsigned bw0[SPL], bw1[SPL];
    SK_UNROLL
    for (int j = 0; j < SPL; ++j) {
        const int m = vit::state_of(lane, j, Ns), p0 = vit::pred0(m, Ns);
        const unsigned u = vit::in_bit(m, K);
        bw0[j] = vit::branch_word(a.gmask, R, K, p0, u);
        bw1[j] = vit::branch_word(a.gmask, R, K, p0 + 1, u);
    }
    const int pl = vit::pred_lane(lane, Ns);

    MT M[SPL];
    uint32_t H[SPL][W];
    MT *st_m = reinterpret_cast<MT *>(a.state);
    uint32_t *st_h = reinterpret_cast<uint32_t *>(static_cast<char *>(a.state) + (size_t)Ns * 8);
    SK_UNROLL
    for (int j = 0; j < SPL; ++j) {
        const int m = vit::state_of(lane, j, Ns);
        const bool carried = a.state != nullptr && active;
        M[j] = carried ? st_m[m * (8 / sizeof(MT))] : MT(0);
        SK_UNROLL
        for (int w = 0; w < W; ++w) H[j][w] = carried ? st_h[m * vit::kMaxWords + w] : 0u;
    }

    // a block: lane `sub` of a stream holds symbols t0 + q GL + sub, q < Q
    auto load_block = [&](int64_t t0, VT(&r)[Q][3]) {
        SK_UNROLL
        for (int q = 0; q < Q; ++q) {
            const int64_t i0 = (t0 + q * GL + sub) * R;
            SK_UNROLL
            for (int k = 0; k < 3; ++k) r[q][k] = (k < R && active && i0 + k < a.nval) ? (VT)x[i0 + k] : pad;
        }
    };
    VT cur[Q][3], nxt[Q][3];
    load_block(0, cur);

    unsigned long long obits = 0;
    int ocnt = 0;
    int64_t obase = 0;

    for (int64_t t0 = 0; t0 < a.nsym; t0 += B) {
        if (t0 + B < a.nsym) load_block(t0 + B, nxt);
        SK_UNROLL
        for (int q = 0; q < Q; ++q) {
            const int64_t tq = t0 + q * GL;
            const int cnt = tq >= a.nsym ? 0 : (a.nsym - tq < GL ? (int)(a.nsym - tq) : GL);
            for (int tt = 0; tt < cnt; ++tt) {
                // the symbol's values, from the lane of this stream that loaded them; each value's distance to both code bits
                VT v[3];
                SK_UNROLL
                for (int k = 0; k < 3; ++k) v[k] = k < 2 || R == 3 ? __shfl(cur[q][k], base + tt) : pad;
                MT d[3][2];
                vit::Dist<METRIC>::both(v, R, a.top, d);

                if constexpr (SPL == 1) {
                    const MT pm0 = __shfl(M[0], pl), pm1 = __shfl(M[0], pl + 1);
                    uint32_t h0[W], h1[W];
                    SK_UNROLL
                    for (int w = 0; w < W; ++w) {
                        h0[w] = __shfl(H[0][w], pl);
                        h1[w] = __shfl(H[0][w], pl + 1);
                    }
                    vit::acs<MT, W>(pm0, pm1, vit::branch_metric<MT>(d, R, bw0[0]), vit::branch_metric<MT>(d, R, bw1[0]), h0, h1,
                                    vit::in_bit(sub, K), &M[0], H[0]);
                } else {
                    // every slot of the two predecessor lanes; this lane's pairs read slot (lane >> 5) + 2 jj of them
                    MT a0[SPL], a1[SPL];
                    uint32_t g0[SPL][W], g1[SPL][W];
                    SK_UNROLL
                    for (int s = 0; s < SPL; ++s) {
                        a0[s] = __shfl(M[s], pl);
                        a1[s] = __shfl(M[s], pl + 1);
                        SK_UNROLL
                        for (int w = 0; w < W; ++w) {
                            g0[s][w] = __shfl(H[s][w], pl);
                            g1[s][w] = __shfl(H[s][w], pl + 1);
                        }
                    }
                    const bool hi = lane >= 32;
                    SK_UNROLL
                    for (int jj = 0; jj < NP; ++jj) {
                        const MT pm0 = hi ? a0[2 * jj + 1] : a0[2 * jj], pm1 = hi ? a1[2 * jj + 1] : a1[2 * jj];
                        uint32_t h0[W], h1[W];
                        SK_UNROLL
                        for (int w = 0; w < W; ++w) {
                            h0[w] = hi ? g0[2 * jj + 1][w] : g0[2 * jj][w];
                            h1[w] = hi ? g1[2 * jj + 1][w] : g1[2 * jj][w];
                        }
                        vit::acs<MT, W>(pm0, pm1, vit::branch_metric<MT>(d, R, bw0[jj]), vit::branch_metric<MT>(d, R, bw1[jj]), h0, h1, 0u,
                                        &M[jj], H[jj]);
                        vit::acs<MT, W>(pm0, pm1, vit::branch_metric<MT>(d, R, bw0[jj + NP]), vit::branch_metric<MT>(d, R, bw1[jj + NP]), h0,
                                        h1, 1u, &M[jj + NP], H[jj + NP]);
                    }
                }

                // the stream's minimum: over this lane's states, then an xor butterfly over the stream's GL lanes
                MT mn = M[0];
                SK_UNROLL
                for (int j = 1; j < SPL; ++j) mn = M[j] < mn ? M[j] : mn;
                SK_UNROLL
                for (int off = 1; off < GL; off <<= 1) {
                    const MT o = __shfl_xor(mn, off);
                    mn = o < mn ? o : mn;
                }
                // the first state attaining it (slot-major = state order) and that state's oldest bit
                unsigned obit = 0;
                bool found = false;
                SK_UNROLL
                for (int j = 0; j < SPL; ++j) {
                    const unsigned long long eq = __ballot(M[j] == mn), hb = __ballot(vit::oldest_bit(H[j], depth) != 0u);
                    unsigned long long e = eq >> base;
                    if (GL < vit::kWave) e &= (1ull << (GL & 63)) - 1ull;
                    if (!found && e != 0ull) {
                        obit = (unsigned)((hb >> (base + __ffsll((long long)e) - 1)) & 1ull);
                        found = true;
                    }
                }
                if constexpr (METRIC != vit::kUnquant) {
                    SK_UNROLL
                    for (int j = 0; j < SPL; ++j) M[j] -= mn;
                }

                if (tq + tt >= depth - 1) {
                    obits |= (unsigned long long)obit << ocnt;
                    if (++ocnt == 64) {
                        if (active) {
                            SK_UNROLL
                            for (int i = sub; i < 64; i += GL) y[obase + i] = (uint8_t)((obits >> i) & 1ull);   // obase + 64 <= nout here
                        }
                        obase += 64;
                        obits = 0;
                        ocnt = 0;
                    }
                }
            }
        }
        if (t0 + B < a.nsym) {
            SK_UNROLL
            for (int q = 0; q < Q; ++q) {
                SK_UNROLL
                for (int k = 0; k < 3; ++k) cur[q][k] = nxt[q][k];
            }
        }
    }
    if (active) {
        for (int i = sub; i < ocnt; i += GL)
            if (obase + i < a.nout) y[obase + i] = (uint8_t)((obits >> i) & 1ull);
    }
    if (a.state != nullptr && active) {
        SK_UNROLL
        for (int j = 0; j < SPL; ++j) {
            const int m = vit::state_of(lane, j, Ns);
            st_m[m * (8 / sizeof(MT))] = M[j];
            SK_UNROLL
            for (int w = 0; w < W; ++w) st_h[m * vit::kMaxWords + w] = H[j][w];
        }
    }
}

struct VitHandle : HandleBase {
    vit::Plan plan;
    DevTable<char> state;    // vit::state_bytes(plan), zero = at rest
    int family = 0;          // whose metrics the state holds: 0 at rest, 1 hard / soft (int32), 2 unquant (float64)
};

template <int METRIC, int K> static void launch_w(int words, unsigned grid, hipStream_t s, const VitArgs &a)
{
    if (words == 2) hipLaunchKernelGGL((viterbi_kernel<METRIC, K, 2>), dim3(grid), dim3(vit::kWave), 0, s, a);
    else hipLaunchKernelGGL((viterbi_kernel<METRIC, K, 4>), dim3(grid), dim3(vit::kWave), 0, s, a);
}
template <int METRIC> static void launch_k(int K, int words, unsigned grid, hipStream_t s, const VitArgs &a)
{
    switch (K) {
    case 3: launch_w<METRIC, 3>(words, grid, s, a); break;
    case 4: launch_w<METRIC, 4>(words, grid, s, a); break;
    case 5: launch_w<METRIC, 5>(words, grid, s, a); break;
    case 6: launch_w<METRIC, 6>(words, grid, s, a); break;
    case 7: launch_w<METRIC, 7>(words, grid, s, a); break;
    case 8: launch_w<METRIC, 8>(words, grid, s, a); break;
    default: launch_w<METRIC, 9>(words, grid, s, a); break;
    }
}

}  // namespace

// argument errors need no device
int viterbi_create(const char *const *polys, int npoly, int depth, HandleBase **out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "viterbi_create: null out");
    vit::Plan plan;
    const char *why = vit::plan_make(polys, npoly, depth, &plan);
    SK_CHECK(!why, SKDSP_ERR_BADARG, "viterbi_create: %s (got %d polynomials, Depth %d)", why, npoly, depth);
    {
        int rc = ensure_init();
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> ctxlk(ctx().mu);
    std::unique_ptr<VitHandle> h(new VitHandle());
    h->kind = H_VITERBI;
    h->dtype = 0;
    h->plan = plan;
    if (int rc = h->state.alloc(vit::state_bytes(plan))) return rc;
    SK_HIP(hipMemsetAsync(h->state.dev, 0, vit::state_bytes(plan), ctx().stream));
    SK_HIP(hipStreamSynchronize(ctx().stream));
    *out = h.release();
    return SKDSP_OK;
}

int viterbi_out_len(HandleBase *hb, int64_t nval, int64_t *n_out)
{
    VitHandle *h = static_cast<VitHandle *>(hb);
    SK_CHECK(n_out && nval >= 0, SKDSP_ERR_BADARG, "viterbi_out_len: bad arguments");
    *n_out = vit::out_len(h->plan, nval);
    return SKDSP_OK;
}

int viterbi_reset(HandleBase *hb, hipStream_t s)
{
    VitHandle *h = static_cast<VitHandle *>(hb);
    SK_HIP(hipMemsetAsync(h->state.dev, 0, vit::state_bytes(h->plan), s));
    h->family = 0;
    return SKDSP_OK;
}

int viterbi_check(HandleBase *hb, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, int stateful)
{
    VitHandle *h = static_cast<VitHandle *>(hb);
    SK_CHECK(metric >= vit::kHard && metric <= vit::kUnquant, SKDSP_ERR_BADARG, "viterbi: metric must be 0 (hard), 1 (soft) or 2 (unquant), got %d", metric);
    SK_CHECK(xtype == metric, SKDSP_ERR_BADARG, "viterbi: hard reads int8, soft int16, unquant float64 values (xtype %d for metric %d)", xtype, metric);
    SK_CHECK(n >= 1 && nrow >= 1, SKDSP_ERR_BADARG, "viterbi: need at least one value and one row (got %lld x %lld)", (long long)nrow, (long long)n);
    SK_CHECK(metric == vit::kHard || n % h->plan.R == 0, SKDSP_ERR_BADARG, "viterbi: %lld values are no multiple of the %d per symbol", (long long)n, h->plan.R);
    SK_CHECK(metric != vit::kSoft || (quant_level >= 0 && quant_level <= vit::kSoftMaxQuant), SKDSP_ERR_BADARG,
             "viterbi: quant_level must be 0 ... %d (got %d)", vit::kSoftMaxQuant, quant_level);
    SK_CHECK(vit::symbols_of(h->plan, n) < ((int64_t)1 << 40) && nrow < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "viterbi: %lld rows of %lld values in one launch",
             (long long)nrow, (long long)n);
    const int family = metric == vit::kUnquant ? 2 : 1;
    SK_CHECK(!stateful || h->family == 0 || h->family == family, SKDSP_ERR_BADARG,
             "viterbi: the carried state holds %s metrics; reset() before decoding with the other metric family", h->family == 2 ? "unquant" : "hard / soft");
    return SKDSP_OK;
}

// x_dev: nrow rows of n values (int8 / int16 / float64 by metric), contiguous; y_dev: nrow rows of out_len(n) bytes.  stateful (one row):
// from and into the handle's carried state.  The soft values must already be truncated and within +-kSoftMaxAbs (the callers' duty).
int viterbi_launch(HandleBase *hb, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y_dev,
                   int stateful, hipStream_t s)
{
    VitHandle *h = static_cast<VitHandle *>(hb);
    int rc = viterbi_check(hb, n, nrow, xtype, metric, quant_level, stateful);
    if (rc) return rc;
    SK_CHECK(!stateful || nrow == 1, SKDSP_ERR_BADARG, "viterbi: the carried state belongs to one stream (got %lld rows)", (long long)nrow);
    const vit::Plan &p = h->plan;
    VitArgs a;
    a.x = x_dev;
    a.y = y_dev;
    a.state = stateful ? h->state.dev : nullptr;
    a.nval = n;
    a.nsym = vit::symbols_of(p, n);
    a.nout = vit::out_len(p, n);
    a.nrow = nrow;
    a.x_stride = n;
    a.y_stride = a.nout;
    a.depth = p.depth;
    a.R = p.R;
    a.top = (1 << quant_level) - 1;
    for (int j = 0; j < 3; ++j) a.gmask[j] = p.gmask[j];
    if (!stateful && a.nout == 0) return SKDSP_OK;
    SK_CHECK(x_dev && (y_dev || a.nout == 0), SKDSP_ERR_BADARG, "viterbi: null pointer");
    const unsigned grid = (unsigned)((nrow + p.streams - 1) / p.streams);
    switch (metric) {
    case vit::kHard: launch_k<vit::kHard>(p.K, p.words, grid, s, a); break;
    case vit::kSoft: launch_k<vit::kSoft>(p.K, p.words, grid, s, a); break;
    default: launch_k<vit::kUnquant>(p.K, p.words, grid, s, a); break;
    }
    SK_HIP(hipGetLastError());
    if (stateful) h->family = metric == vit::kUnquant ? 2 : 1;
    note_path("viterbi");
    return SKDSP_OK;
}

}  // namespace skdsp
