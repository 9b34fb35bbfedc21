// iir_scan.hip -- exact parallel IIR (cascaded DF2T sections) for gfx950 (MI355X).
//
// Serves  scipy.signal.sosfilt(sos,x)   multirate_helper.py:173,182,190 (multirate_IIR)
//         scipy.signal.lfilter(b,a,x)   multirate_helper.py:74,81        (rate_change; the
//                                       transfer function is factored into biquads by iir_api.hip)
// with zero initial state, as the reference always calls them.
//
// The recurrence is serial in n, so the signal is cut into J contiguous chunks of T
// samples, ONE CHUNK PER THREAD (J ~ 128 Ki threads on 256 CUs), and made exact with an
// affine scan over the D-dimensional filter state (D = sections x order <= 24):
//     s_out = M s_in + v ,   M = A^T (one-chunk transition),  v = zero-state end state
//   K1  every thread runs the cascade over its chunk from zero state -> v_j ; the
//       workgroup tree-reduces its 256 v_j (matrix powers M^(2^l)) into one aggregate
//       (decaying filters with <= 8 biquads: v = G x on the FP64 matrix pipe instead, and the
//       carries straight from the v_j -- iir_k1_mfma_kernel / iir_carry_kernel below)
//   K2  one workgroup scans the <=512 workgroup aggregates (powers M^(256*2^l)); skipped when
//       (M^256)^k underflows within 8 powers (any ordinary stable filter): K3 then sums the
//       few significant look-back terms itself
//   K3  every workgroup scans its 256 v_j seeded with its carry-in, then every thread
//       re-runs the cascade from its now-exact initial state and writes y
// Scan levels whose matrix power M^(2^l) has every entry below 1e-30 are skipped (their term is
// far under one ulp of the float64 recurrence), and every matvec uses the block lower-triangular
// shape of a cascade's transition powers.
// Nothing is approximated (no "warm-up overlap"): marginally stable / slowly decaying
// filters are handled exactly.  State, coefficients, matrix powers and accumulation
// are float64 on-chip for every signal dtype -- a float32 recurrence sits at 1e-6 of
// the float64 reference already when run sequentially, so float32
// I/O with float64 state is the only way to hold the 1e-6 parity bound.
//
// HBM: x is read twice (K1, K3), y written once, v_j costs 8*D bytes per chunk.
// A thread walks its chunk sequentially, which would be uncoalesced, so each
// workgroup stages a [256 chunks x 32 samples] piece through LDS with full-line
// 16-byte loads (row pitch 36 floats / 34 doubles: conflict-free ds_read_b128), and
// prefetches the next piece into registers while it computes the current one.
// FP64 VALU is the busy unit (40 dependent-ish v_fma_f64 per sample for 8 biquads);
// algorithmic bytes = 8 B per f32 sample (4 in + 4 out).
#include "iir_common.hpp"


// SK_SCAN_PART: this file is compiled twice so that its ~150 kernel instantiations (the long pole of the build: 136 s in one
// piece) compile side by side: 1 = host side + the float32 kernels (build/iir_scan.o), 2 = the float64 kernels and their dispatch
// only (build/iir_scan_f64.o); 0 = everything in one object (variant builds)
#ifndef SK_SCAN_PART
#define SK_SCAN_PART 0
#endif

namespace skdsp {

struct IirArgs {
    const void *x;
    void *y;
    int64_t n;
    int64_t T;        // chunk length (multiple of 32)
    int64_t J;        // number of chunks
    int64_t batch_stride;  // elements between batch items (planar complex = 2 items)
    int il;               // 1: x / y are interleaved complex (aggregate-free mode only; iir_k1c / iir_k3c kernels)
    const double *pw; // matrix powers
    double *v;        // [batch][D][J]
    double *agg;      // [batch][W][D]  workgroup aggregates (K1 out)
    const double *carry;  // [batch][W][D]  workgroup carry-in (K3 in), used when n_lb == 0
    const double *lbmat;  // [n_lb-1][D][D]: (M^256)^k, k = 1..n_lb-1
    int n_lb;             // > 0: carry = sum_{k<n_lb} (M^256)^k agg[wg-1-k] computed in K3 (no K2 launch)
    int n_lv;             // chunk-level scan levels whose power M^(2^l) is not yet negligible (<= 8)
    const double *zi;     // [batch][D] initial state (streaming; null = rest, what the reference uses)
    double *zf;           // [batch][D] state after sample n-1 (null = not wanted)
    int dec;              // > 1: K3 stores only y[k * dec] (at y[k]), k < n_keep / dec  (.dn: no full-rate result in HBM)
    int dec_dq, dec_dr;   // (32 T) div / mod dec: index step between a thread's staged segments
    int64_t n_keep;       // (n / dec) * dec
};

// Kernel body shared by K1 (WRITE=false) and K3 (WRITE=true).
template <int NSEC, int ORD, typename IO, bool WRITE, bool UNIT = false>
__global__ __launch_bounds__(kIirThreads) void iir_chunk_kernel(IirArgs a, Coef<NSEC, ORD> cf)
{
    constexpr int D = NSEC * ORD;
    using St = Stage<IO>;
    constexpr int kStageBytes = kIirThreads * St::pitch * (int)sizeof(IO);
    constexpr int kScanBytes = kIirThreads * D * 8;
    constexpr int kLdsBytes = kStageBytes > kScanBytes ? kStageBytes : kScanBytes;
    __shared__ __attribute__((aligned(16))) char lds_raw[kLdsBytes];
    IO *stage = reinterpret_cast<IO *>(lds_raw);
    double *sc = reinterpret_cast<double *>(lds_raw);

    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x;
    const int bat = blockIdx.y;
    const int64_t W = gridDim.x;
    const int64_t cj = wg * kIirThreads + tid;  // my chunk
    const IO *x = reinterpret_cast<const IO *>(a.x) + (size_t)bat * a.batch_stride;
    IO *y = reinterpret_cast<IO *>(a.y) + (size_t)bat * a.batch_stride;
    double *vbase = a.v + (size_t)bat * D * a.J;

    double z[D];
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] = 0.0;

    if (WRITE) {
        // ---- seeded inclusive Hillis-Steele scan of the workgroup's 256 chunk maps ----
        double v[D];
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = (cj < a.J) ? vbase[(size_t)d * a.J + cj] : 0.0;
        double c0[D];  // carry-in of this workgroup (only thread 0 needs it)
#pragma unroll
        for (int d = 0; d < D; ++d) c0[d] = 0.0;
        if (tid == 0) {
            if (a.n_lb > 0) {
                // short look-back: the workgroup-level transition (M^256) of a stable filter
                // underflows after a few powers, so the carry is a handful of terms
                const double *ag = a.agg + (size_t)bat * W * D;
                if (wg >= 1) {
#pragma unroll
                    for (int d = 0; d < D; ++d) c0[d] = ag[(size_t)(wg - 1) * D + d];
                }
                for (int k = 1; k < a.n_lb; ++k) {
                    if (wg - 1 - k < 0) break;
                    double tmp[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) tmp[d] = ag[(size_t)(wg - 1 - k) * D + d];
                    matvec_acc<D, ORD>(a.lbmat + (size_t)(k - 1) * D * D, tmp, c0);
                }
                if (a.zi && wg < a.n_lb) {  // the initial state reaches workgroup wg as (M^256)^wg zi
                    double tmp[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) tmp[d] = a.zi[(size_t)bat * D + d];
                    if (wg == 0) {
#pragma unroll
                        for (int d = 0; d < D; ++d) c0[d] += tmp[d];
                    } else {
                        matvec_acc<D, ORD>(a.lbmat + (size_t)(wg - 1) * D * D, tmp, c0);
                    }
                }
            } else {
                const double *cin = a.carry + ((size_t)bat * W + wg) * D;
#pragma unroll
                for (int d = 0; d < D; ++d) c0[d] = cin[d];
            }
            matvec_acc<D, ORD>(a.pw, c0, v);  // v0' = M carry + v0
        }
#pragma unroll 1
        for (int l = 0; l < a.n_lv; ++l) {
            const int s = 1 << l;
#pragma unroll
            for (int d = 0; d < D; ++d) sc[d * kIirThreads + tid] = v[d];
            __syncthreads();
            if (tid >= s) {
                double left[D];
#pragma unroll
                for (int d = 0; d < D; ++d) left[d] = sc[d * kIirThreads + tid - s];
                matvec_acc<D, ORD>(a.pw + (size_t)l * D * D, left, v);
            }
            __syncthreads();
        }
        // exclusive: my initial state = inclusive state of the chunk to my left
#pragma unroll
        for (int d = 0; d < D; ++d) sc[d * kIirThreads + tid] = v[d];
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] = c0[d];
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] = sc[d * kIirThreads + tid - 1];
        }
        __syncthreads();
    }

    // streaming: the thread that owns sample n-1 publishes its state right after that sample
    const bool zf_owner = WRITE && a.zf != nullptr && cj == (a.n - 1) / a.T;
    const int zf_off = (int)((a.n - 1) % a.T);
    const int zf_piece = (WRITE && a.zf != nullptr) ? zf_off / kPiece : -1;  // uniform

    // ---- walk the chunk in staged pieces of 32 samples per thread ----
    const int64_t row0 = wg * kIirThreads;  // first chunk (row) of this workgroup
    const int npieces = (int)(a.T / kPiece);
    // Workgroups whose 256 chunks lie inside the signal (all but the last one or two) prefetch with unguarded
    // 16-byte loads; the others stage each piece synchronously by their own code.  (One load routine with
    // per-lane guards put every prefetch load into its own branch region, and hipcc waits for it at the merge:
    // vmcnt(0) right behind each load = no prefetch at all.)
    const bool interior = (row0 + kIirThreads) * a.T <= a.n;
    typedef float pre_t __attribute__((ext_vector_type(4)));  // (a struct float4 here ends up as memcpy into scratch)
    pre_t pre[St::per_thread];
    auto load_piece = [&](int p) {  // interior workgroups only
#pragma unroll
        for (int i = 0; i < St::per_thread; ++i) {
            const int idx = i * kIirThreads + tid;
            const int row = idx / St::segs, seg = idx % St::segs;
            const int64_t g = (row0 + row) * a.T + (int64_t)p * kPiece + (int64_t)seg * St::elems;  // element index
            pre[i] = *reinterpret_cast<const pre_t *>(x + g);
        }
    };
    auto stage_slow = [&](int p) {  // zero beyond the signal
#pragma unroll 1
        for (int i = 0; i < St::per_thread; ++i) {
            const int idx = i * kIirThreads + tid;
            const int row = idx / St::segs, seg = idx % St::segs;
            const int64_t g = (row0 + row) * a.T + (int64_t)p * kPiece + (int64_t)seg * St::elems;
            IO *dst = stage + row * St::pitch + seg * St::elems;
#pragma unroll
            for (int e = 0; e < St::elems; ++e) dst[e] = (g + e < a.n) ? x[g + e] : IO(0);
        }
    };
    if (interior) load_piece(0);
#pragma unroll 1
    for (int p = 0; p < npieces; ++p) {
        if (interior) {
#pragma unroll
            for (int i = 0; i < St::per_thread; ++i) {
                const int idx = i * kIirThreads + tid;
                const int row = idx / St::segs, seg = idx % St::segs;
                *reinterpret_cast<pre_t *>(stage + row * St::pitch + seg * St::elems) = pre[i];
            }
        } else {
            stage_slow(p);
        }
        __syncthreads();
        if (interior && p + 1 < npieces) load_piece(p + 1);  // in flight while this piece is computed
        IO *myrow = stage + tid * St::pitch;
        auto run_piece = [&](auto capture) {
#pragma unroll
            for (int sgi = 0; sgi < St::segs; ++sgi) {
                float4 raw = *reinterpret_cast<const float4 *>(myrow + sgi * St::elems);
                IO *e4 = reinterpret_cast<IO *>(&raw);
#pragma unroll
                for (int e = 0; e < St::elems; ++e) {
                    const double yv = cascade_step<NSEC, ORD, UNIT>(cf, z, (double)e4[e]);
                    if (WRITE) e4[e] = (IO)yv;
                    if (decltype(capture)::value && zf_owner && sgi * St::elems + e == zf_off % kPiece) {
#pragma unroll
                        for (int d = 0; d < D; ++d) a.zf[(size_t)bat * D + d] = z[d];
                    }
                }
                if (WRITE) *reinterpret_cast<float4 *>(myrow + sgi * St::elems) = raw;
            }
        };
        if (WRITE && p == zf_piece) run_piece(std::true_type{});  // the one piece that holds sample n-1
        else run_piece(std::false_type{});
        if (WRITE) {
            __syncthreads();
            int64_t dq_run = 0;
            int dr_run = 0;
#pragma unroll
            for (int i = 0; i < St::per_thread; ++i) {
                const int idx = i * kIirThreads + tid;
                const int row = idx / St::segs, seg = idx % St::segs;
                const int64_t g = (row0 + row) * a.T + (int64_t)p * kPiece + (int64_t)seg * St::elems;
                const float4 val = *reinterpret_cast<const float4 *>(stage + row * St::pitch + seg * St::elems);
                if (a.dec > 1) {
                    // decimating store: segment i of this thread starts 32 T samples after segment i - 1, so its
                    // (quotient, remainder) by dec follow from the first one by adding (dec_dq, dec_dr)
                    if (i == 0) {
                        dq_run = g / a.dec;
                        dr_run = (int)(g - dq_run * a.dec);
                    }
                    const IO *tmp = reinterpret_cast<const IO *>(&val);
                    if (a.dec >= St::elems) {  // at most one kept sample per 16-byte segment: one store
                        const int e0 = dr_run == 0 ? 0 : a.dec - dr_run;
                        if (e0 < St::elems && g + e0 < a.n_keep) {
                            IO pick = tmp[0];
#pragma unroll
                            for (int e = 1; e < St::elems; ++e) pick = (e0 == e) ? tmp[e] : pick;
                            y[dq_run + (dr_run != 0)] = pick;
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < St::elems; ++e) {
                            const int t = dr_run + e;  // < dec + elems
                            const int m = (t >= a.dec) + (t >= 2 * a.dec) + (t >= 3 * a.dec) + (t >= 4 * a.dec);
                            if (t == m * a.dec && g + e < a.n_keep) y[dq_run + m] = tmp[e];
                        }
                    }
                    dq_run += a.dec_dq;
                    dr_run += a.dec_dr;
                    if (dr_run >= a.dec) { dr_run -= a.dec; ++dq_run; }
                } else if (interior || g + St::elems <= a.n) {
                    {
                        typedef float nt4_t __attribute__((ext_vector_type(4)));
                        nt4_t q = {val.x, val.y, val.z, val.w};
                        __builtin_nontemporal_store(q, reinterpret_cast<nt4_t *>(y + g));
                    }
                } else if (g < a.n) {
                    const IO *tmp = reinterpret_cast<const IO *>(&val);
#pragma unroll
                    for (int e = 0; e < St::elems; ++e)
                        if (g + e < a.n) y[g + e] = tmp[e];
                }
            }
        }
        __syncthreads();
    }

    if (!WRITE) {
        // ---- chunk end states to HBM (SoA, coalesced) + workgroup tree reduction ----
        if (cj < a.J) {
#pragma unroll
            for (int d = 0; d < D; ++d) vbase[(size_t)d * a.J + cj] = z[d];
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] = 0.0;
        }
#pragma unroll 1
        for (int l = 0; l < a.n_lv; ++l) {
            const int s = 1 << l;
#pragma unroll
            for (int d = 0; d < D; ++d) sc[d * kIirThreads + tid] = z[d];
            __syncthreads();
            if ((tid & (2 * s - 1)) == 2 * s - 1) {
                double left[D];
#pragma unroll
                for (int d = 0; d < D; ++d) left[d] = sc[d * kIirThreads + tid - s];
                matvec_acc<D, ORD>(a.pw + (size_t)l * D * D, left, z);
            }
            __syncthreads();
        }
        if (tid == kIirThreads - 1) {
            double *out = a.agg + ((size_t)bat * W + wg) * D;
#pragma unroll
            for (int d = 0; d < D; ++d) out[d] = z[d];
        }
    }
}

// K1 as a matrix product (aggregate-free mode only).  From rest, the state at the end of a chunk is
// linear in its T samples:  v = sum_k A^(T-1-k) b x_k = G x  with G a D x T matrix that depends on the
// filter and on T alone -- 2*D flop per sample instead of the 5 dependent FMA per biquad of the
// recurrence, and a dense FP64 contraction, so it runs on the matrix pipe: one wave owns 16 chunks and
// accumulates  V[16 states x 16 chunks] += G[:, 4 samples] * X[4 samples, 16 chunks]  with
// v_mfma_f64_16x16x4_f64 (A operand: lane l holds G[l & 15][k0 + (l >> 4)], B operand: lane l holds
// x[chunk l & 15][k0 + (l >> 4)]; C: col = lane & 15, row = (lane >> 4) + 4 reg).  The samples of the
// wave's 16 chunks are staged per 128-sample piece in a wave-private LDS image (row pitch 132 words:
// the 64 B-operand reads of a step hit 64 distinct banks), so there is no workgroup barrier at all.
constexpr int kMmPiece = 128;                 // samples of every chunk staged at a time
constexpr int kMmPitch = kMmPiece + 4;        // in 4-byte words (float); doubles use 2 words per sample

// NT = 1: D <= 16 states (<= 8 biquads); NT = 2: up to 32 states in two 16-row tiles sharing the B operand.
template <typename IO, int NT>
__global__ __launch_bounds__(256) void iir_k1_mfma_kernel(const IO *__restrict__ xin, int64_t n, int64_t T, int64_t J,
                                                          int64_t batch_stride, const double *__restrict__ Gt,
                                                          double *__restrict__ vout, int D)
{
    constexpr int E = 16 / (int)sizeof(IO);               // samples per 16-byte load
    constexpr int W = (int)sizeof(IO) / 4;                // 4-byte words per sample
    constexpr int kLoads = 16 * kMmPiece / E / 64;        // 16-byte loads per lane per piece
    __shared__ __attribute__((aligned(16))) float lds[4 * 16 * kMmPitch * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bat = blockIdx.y;
    const IO *x = xin + (size_t)bat * batch_stride;
    double *vbase = vout + (size_t)bat * D * J;
    float *img = lds + wave * (16 * kMmPitch * W);
    const int64_t chunk0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (chunk0 >= J) return;
    const int npieces = (int)(T / kMmPiece);
    // waves whose 16 chunks lie inside the signal prefetch with unguarded 16-byte loads; the last wave or two stage
    // every piece synchronously by their own code (per-lane guards around the loads = a vmcnt(0) behind each of them)
    const bool interior = (chunk0 + 16) * T <= n;
    typedef float pre_t __attribute__((ext_vector_type(4)));
    pre_t pre[kLoads];
    auto load_piece = [&](int p) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;                    // 16-byte segment of the 16 x piece image
            const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
            const int64_t g = (chunk0 + row) * T + (int64_t)p * kMmPiece + (int64_t)seg * E;
            pre[i] = *reinterpret_cast<const pre_t *>(x + g);
        }
    };
    auto stage_slow = [&](int p) {
#pragma unroll 1
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
            const int64_t g = (chunk0 + row) * T + (int64_t)p * kMmPiece + (int64_t)seg * E;
            IO *dst = reinterpret_cast<IO *>(img) + row * kMmPitch + seg * E;
#pragma unroll
            for (int e = 0; e < E; ++e) dst[e] = (g + e < n) ? x[g + e] : IO(0);
        }
    };
    v4d_t acc0[NT], acc1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc0[t] = acc1[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, j = lane >> 4;
    const size_t tstride = (size_t)(T / 4) * 64;  // doubles per row tile of the table
    if (interior) load_piece(0);
    for (int p = 0; p < npieces; ++p) {
        if (interior) {
#pragma unroll
            for (int i = 0; i < kLoads; ++i) {
                const int idx = i * 64 + lane;
                const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
                *reinterpret_cast<pre_t *>(img + (row * kMmPitch + seg * E) * W) = pre[i];
            }
        } else {
            stage_slow(p);
        }
        // The A operands stream from the L2-resident table inside the step loop; the HBM loads of the next
        // piece are requested only AFTER the loop: vmcnt retires in order, so table loads queued behind a
        // prefetch would wait for HBM at every step.  Four waves per SIMD cover the exposed latency.
        const double *gt = Gt + ((size_t)p * (kMmPiece / 4)) * 64 + lane;
        const IO *xs = reinterpret_cast<const IO *>(img) + c * kMmPitch + j;
#pragma unroll 8
        for (int s = 0; s < kMmPiece / 4; s += 2) {
            const double b0 = (double)xs[4 * s], b1 = (double)xs[4 * s + 4];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc0[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[t * tstride + (size_t)s * 64], b0, acc0[t], 0, 0, 0);
                acc1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[t * tstride + (size_t)(s + 1) * 64], b1, acc1[t], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory");
        if (interior && p + 1 < npieces) load_piece(p + 1);
    }
    const int64_t cj = chunk0 + c;
    if (cj < J) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * t + j + 4 * r;
                if (d < D) vbase[(size_t)d * J + cj] = acc0[t][r] + acc1[t][r];
            }
    }
}

// Aggregate-free carries: when M^32 is negligible the state entering workgroup w is
//   carry[w] = sum_{k<32} M^k v[256 w - 1 - k]        (chunk -1 holds the caller's initial state)
// One small workgroup per w: thread (k = tid & 31, row pair tid >> 5) applies two rows of its own power
// M^k from the lane-contiguous table lbk[i][j][k]; a half-wave shuffle tree sums over k.
template <int D, int ORD>
__global__ __launch_bounds__(256) void iir_carry_kernel(const double *__restrict__ v, const double *__restrict__ lbk, int64_t J,
                                                        const double *__restrict__ zi, double *__restrict__ carry)
{
    const int tid = threadIdx.x, k = tid & 31;
    const int64_t w = blockIdx.x, W = gridDim.x;
    const int bat = blockIdx.y;
    const double *vbase = v + (size_t)bat * D * J;
    const int64_t ck = w * kIirThreads - 1 - k;
#pragma unroll 1
    for (int i0 = (tid >> 5) * ORD; i0 < D; i0 += 8 * ORD) {
    double r[ORD];
#pragma unroll
    for (int q = 0; q < ORD; ++q) r[q] = 0.0;
    {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j < i0 + ORD) {
                double u = 0.0;
                if (ck >= 0) u = vbase[(size_t)j * J + ck];
                else if (ck == -1 && zi) u = zi[(size_t)bat * D + j];
#pragma unroll
                for (int q = 0; q < ORD; ++q) r[q] = fma(lbk[((size_t)(i0 + q) * D + j) * 32 + k], u, r[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < ORD; ++q) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) r[q] += __shfl_xor(r[q], m);
    }
    if (k == 0) {
#pragma unroll
        for (int q = 0; q < ORD; ++q) carry[((size_t)bat * W + w) * D + i0 + q] = r[q];
    }
    }
}

// K1 with the end-state map G in REGISTERS (chunks of 128, 256 or 512 samples, <= 16 states): wave w keeps the 32
// A operands of piece w % NP for the whole launch and walks groups of 16 chunks; the partial products of the NP
// pieces of a chunk group are summed through LDS.  Without table loads in the step loop the prefetch of the next
// group's samples can be issued BEFORE the MFMAs (vmcnt retires in order: table loads queued behind a prefetch
// would wait for HBM at every step, which is why iir_k1_mfma_kernel requests its samples only after the loop).
template <typename IO, int NP>
__global__ __launch_bounds__(256) void iir_k1r_kernel(const IO *__restrict__ xin, int64_t n, int64_t J, int64_t batch_stride,
                                                      const double *__restrict__ Gt, double *__restrict__ vout, int D)
{
    constexpr int T = kMmPiece * NP;
    constexpr int E = 16 / (int)sizeof(IO);
    constexpr int W = (int)sizeof(IO) / 4;
    constexpr int kLoads = 16 * kMmPiece / E / 64;
    constexpr int GPW = 4 / NP;  // chunk groups a workgroup works on at a time
    __shared__ __attribute__((aligned(16))) float lds[4 * 16 * kMmPitch * W];
    __shared__ double part[2][4][64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int piece = wave % NP, sub = wave / NP;
    const int bat = blockIdx.y;
    const IO *x = xin + (size_t)bat * batch_stride;
    double *vbase = vout + (size_t)bat * D * J;
    float *img = lds + wave * (16 * kMmPitch * W);
    const int64_t ngroups = (J + 15) / 16;
    const int64_t niter = (ngroups + (int64_t)gridDim.x * GPW - 1) / ((int64_t)gridDim.x * GPW);

    double areg[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) areg[s] = Gt[((size_t)piece * 32 + s) * 64 + lane];

    typedef float pre_t __attribute__((ext_vector_type(4)));
    pre_t pre[kLoads];
    auto group_of = [&](int64_t it) { return (it * gridDim.x + blockIdx.x) * GPW + sub; };
    auto interior = [&](int64_t g) { return g < ngroups && (16 * g + 16) * (int64_t)T <= n; };
    auto load_piece = [&](int64_t g) {  // interior groups only
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
            const int64_t e = (16 * g + row) * T + (int64_t)piece * kMmPiece + (int64_t)seg * E;
            pre[i] = *reinterpret_cast<const pre_t *>(x + e);
        }
    };
    auto stage_slow = [&](int64_t g) {
#pragma unroll 1
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
            const int64_t e = (16 * g + row) * T + (int64_t)piece * kMmPiece + (int64_t)seg * E;
            IO *dst = reinterpret_cast<IO *>(img) + row * kMmPitch + seg * E;
#pragma unroll
            for (int k = 0; k < E; ++k) dst[k] = (e + k < n) ? x[e + k] : IO(0);
        }
    };
    const int c = lane & 15, j = lane >> 4;
    bool fast = interior(group_of(0));
    if (fast) load_piece(group_of(0));
#pragma unroll 1
    for (int64_t it = 0; it < niter; ++it) {
        const int64_t g = group_of(it);
        if (fast) {
#pragma unroll
            for (int i = 0; i < kLoads; ++i) {
                const int idx = i * 64 + lane;
                const int row = idx / (kMmPiece / E), seg = idx % (kMmPiece / E);
                *reinterpret_cast<pre_t *>(img + (row * kMmPitch + seg * E) * W) = pre[i];
            }
        } else if (g < ngroups) {
            stage_slow(g);
        }
        const int64_t gn = group_of(it + 1);
        fast = it + 1 < niter && interior(gn);
        if (fast) load_piece(gn);  // in flight during the MFMAs below
        v4d_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        if (g < ngroups) {
            const IO *xs = reinterpret_cast<const IO *>(img) + c * kMmPitch + j;
#pragma unroll
            for (int s = 0; s < 32; s += 2) {
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[s], (double)xs[4 * s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[s + 1], (double)xs[4 * s + 4], acc1, 0, 0, 0);
            }
        }
        const v4d_t acc = acc0 + acc1;
        double *mine = part[it & 1][wave] + lane * 4;
        if (NP > 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[r] = acc[r];
            __syncthreads();  // (one barrier per iteration: the partial buffers alternate)
        }
        if (piece == 0 && g < ngroups) {
            double sum[4] = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
            for (int q = 1; q < NP; ++q) {
                const double *other = part[it & 1][wave + q] + lane * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[r] += other[r];
            }
            const int64_t cj = 16 * g + c;
            if (cj < J) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int d = j + 4 * r;
                    if (d < D) vbase[(size_t)d * J + cj] = sum[r];
                }
            }
        }
    }
}

// ---- interleaved complex signals, aggregate-free mode: no planes ---------------------------------
// A complex signal through a real-coefficient cascade is two independent real recurrences.  The
// planar detour (deinterleave -> 2 planes -> interleave) costs two extra passes over the signal
// (0.19 ms each at 2^26 complex64, next to 0.45 ms of scan work).  Here the matrix-pipe K1 picks re /
// im out of the interleaved samples as its two B operands, and K3 keeps BOTH states of a chunk in one
// thread: it stages 16-sample (float) / 8-sample (double) complex pieces as two real planes in LDS,
// runs the two recurrences interleaved (twice the ILP of the real kernel) and writes interleaved y.
template <typename IO, int NT>
__global__ __launch_bounds__(256) void iir_k1c_mfma_kernel(const IO *__restrict__ x, int64_t n, int64_t T, int64_t J,
                                                           const double *__restrict__ Gt, double *__restrict__ vout, int D)
{
    constexpr int PCX = 64;                                // complex samples of every chunk staged at a time
    constexpr int PITCH = PCX + 4;                         // complex elements per row (8 / 16 words mod 32: conflict-free)
    constexpr int E = 8 / (int)sizeof(IO);                 // complex samples per 16-byte load (2 float, 1 double)
    constexpr int kLoads = 16 * PCX / E / 64;
    __shared__ __attribute__((aligned(16))) IO lds[4 * 16 * PITCH * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    IO *img = lds + wave * (16 * PITCH * 2);
    const int64_t chunk0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (chunk0 >= J) return;
    const int npieces = (int)(T / PCX);
    const bool interior = (chunk0 + 16) * T <= n;  // (see iir_k1_mfma_kernel)
    typedef float pre_t __attribute__((ext_vector_type(4)));
    pre_t pre[kLoads];
    auto load_piece = [&](int p) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / (PCX / E), seg = idx % (PCX / E);
            const int64_t g = (chunk0 + row) * T + (int64_t)p * PCX + (int64_t)seg * E;  // complex index
            pre[i] = *reinterpret_cast<const pre_t *>(x + 2 * g);
        }
    };
    auto stage_slow = [&](int p) {
#pragma unroll 1
        for (int i = 0; i < kLoads; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / (PCX / E), seg = idx % (PCX / E);
            const int64_t g = (chunk0 + row) * T + (int64_t)p * PCX + (int64_t)seg * E;
            IO *dst = img + (row * PITCH + seg * E) * 2;
#pragma unroll
            for (int e = 0; e < 2 * E; ++e) dst[e] = (g + e / 2 < n) ? x[2 * g + e] : IO(0);
        }
    };
    v4d_t ar0[NT], ar1[NT], ai0[NT], ai1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) ar0[t] = ar1[t] = ai0[t] = ai1[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, j = lane >> 4;
    const size_t tstride = (size_t)(T / 4) * 64;
    if (interior) load_piece(0);
    for (int p = 0; p < npieces; ++p) {
        if (interior) {
#pragma unroll
            for (int i = 0; i < kLoads; ++i) {
                const int idx = i * 64 + lane;
                const int row = idx / (PCX / E), seg = idx % (PCX / E);
                *reinterpret_cast<pre_t *>(img + (row * PITCH + seg * E) * 2) = pre[i];
            }
        } else {
            stage_slow(p);
        }
        const double *gt = Gt + ((size_t)p * (PCX / 4)) * 64 + lane;
        const IO *xs = img + (c * PITCH + j) * 2;
#pragma unroll 8
        for (int s = 0; s < PCX / 4; s += 2) {
            const double br0 = (double)xs[8 * s], bi0 = (double)xs[8 * s + 1];
            const double br1 = (double)xs[8 * s + 8], bi1 = (double)xs[8 * s + 9];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double g0 = gt[t * tstride + (size_t)s * 64], g1 = gt[t * tstride + (size_t)(s + 1) * 64];
                ar0[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(g0, br0, ar0[t], 0, 0, 0);
                ai0[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(g0, bi0, ai0[t], 0, 0, 0);
                ar1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(g1, br1, ar1[t], 0, 0, 0);
                ai1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(g1, bi1, ai1[t], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory");
        if (interior && p + 1 < npieces) load_piece(p + 1);
    }
    const int64_t cj = chunk0 + c;
    if (cj < J) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * t + j + 4 * r;
                if (d < D) {
                    vout[(size_t)d * J + cj] = ar0[t][r] + ar1[t][r];
                    vout[(size_t)(D + d) * J + cj] = ai0[t][r] + ai1[t][r];
                }
            }
    }
}

template <int NSEC, int ORD, typename IO, bool UNIT = false>
__global__ __launch_bounds__(kIirThreads) __attribute__((amdgpu_waves_per_eu(NSEC <= 8 ? 2 : 1, NSEC <= 8 ? 2 : 1))) void iir_k3c_kernel(IirArgs a, Coef<NSEC, ORD> cf)
{
    constexpr int D = NSEC * ORD;
    constexpr int E = 16 / (int)sizeof(IO);      // scalars per 16 bytes
    constexpr int PC = 4 * E;                    // complex samples per staged row piece (128 bytes interleaved)
    constexpr int PITCH = 80 / (int)sizeof(IO);  // scalars per plane row: 80 bytes (conflict-free b128 reads)
    constexpr int kStageBytes = 2 * kIirThreads * 80;
    constexpr int kScanBytes = kIirThreads * D * 8;
    constexpr int kLdsBytes = kStageBytes > kScanBytes ? kStageBytes : kScanBytes;
    __shared__ __attribute__((aligned(16))) char lds_raw[kLdsBytes];
    IO *st_re = reinterpret_cast<IO *>(lds_raw);
    IO *st_im = st_re + kIirThreads * PITCH;
    double *sc = reinterpret_cast<double *>(lds_raw);

    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x, W = gridDim.x;
    const int64_t cj = wg * kIirThreads + tid;
    const IO *x = reinterpret_cast<const IO *>(a.x);
    IO *y = reinterpret_cast<IO *>(a.y);

    // ---- initial states of my chunk for both components: seeded Hillis-Steele scan, twice ----
    double z0[D], z1[D];
    auto scan_plane = [&](int bat, double (&z)[D]) {
        const double *vbase = a.v + (size_t)bat * D * a.J;
        double v[D];
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = (cj < a.J) ? vbase[(size_t)d * a.J + cj] : 0.0;
        double c0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) c0[d] = 0.0;
        if (tid == 0) {
            const double *cin = a.carry + ((size_t)bat * W + wg) * D;
#pragma unroll
            for (int d = 0; d < D; ++d) c0[d] = cin[d];
            matvec_acc<D, ORD>(a.pw, c0, v);
        }
#pragma unroll 1
        for (int l = 0; l < a.n_lv; ++l) {
            const int s = 1 << l;
#pragma unroll
            for (int d = 0; d < D; ++d) sc[d * kIirThreads + tid] = v[d];
            __syncthreads();
            if (tid >= s) {
                double left[D];
#pragma unroll
                for (int d = 0; d < D; ++d) left[d] = sc[d * kIirThreads + tid - s];
                matvec_acc<D, ORD>(a.pw + (size_t)l * D * D, left, v);
            }
            __syncthreads();
        }
#pragma unroll
        for (int d = 0; d < D; ++d) sc[d * kIirThreads + tid] = v[d];
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] = c0[d];
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) z[d] = sc[d * kIirThreads + tid - 1];
        }
        __syncthreads();
    };
    scan_plane(0, z0);
    scan_plane(1, z1);

    const bool zf_owner = a.zf != nullptr && cj == (a.n - 1) / a.T;
    const int zf_off = (int)((a.n - 1) % a.T);
    const int zf_piece = a.zf != nullptr ? zf_off / PC : -1;

    const int64_t row0 = wg * kIirThreads;
    const int npieces = (int)(a.T / PC);
    const bool interior = (row0 + kIirThreads) * a.T <= a.n;  // (see iir_chunk_kernel)
    typedef float pre_t __attribute__((ext_vector_type(4)));
    pre_t pre[8];
    auto load_piece = [&](int p) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = i * kIirThreads + tid;
            const int row = idx >> 3, seg = idx & 7;           // 8 x 16-byte segments per 128-byte row piece
            const int64_t g = (row0 + row) * a.T + (int64_t)p * PC + (int64_t)seg * (E / 2);  // complex index
            pre[i] = *reinterpret_cast<const pre_t *>(x + 2 * g);
        }
    };
    auto split_store = [&](const IO *e, int row, int seg) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < E / 2; ++k) {
            st_re[row * PITCH + seg * (E / 2) + k] = e[2 * k];
            st_im[row * PITCH + seg * (E / 2) + k] = e[2 * k + 1];
        }
    };
    auto stage_slow = [&](int p) {
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const int idx = i * kIirThreads + tid;
            const int row = idx >> 3, seg = idx & 7;
            const int64_t g = (row0 + row) * a.T + (int64_t)p * PC + (int64_t)seg * (E / 2);
            IO tmp[E];
#pragma unroll
            for (int e = 0; e < E; ++e) tmp[e] = (g + e / 2 < a.n) ? x[2 * g + e] : IO(0);
            split_store(tmp, row, seg);
        }
    };
    if (interior) load_piece(0);
#pragma unroll 1
    for (int p = 0; p < npieces; ++p) {
        if (interior) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int idx = i * kIirThreads + tid;
                split_store(reinterpret_cast<const IO *>(&pre[i]), idx >> 3, idx & 7);
            }
        } else {
            stage_slow(p);
        }
        __syncthreads();
        if (interior && p + 1 < npieces) load_piece(p + 1);
        IO *rr = st_re + tid * PITCH, *ri = st_im + tid * PITCH;
        auto run_plane = [&](auto capture, IO *r, double (&z)[D], double *zf) __attribute__((always_inline)) {
#pragma unroll
            for (int c4 = 0; c4 < PC / E; ++c4) {
                float4 raw = *reinterpret_cast<const float4 *>(r + c4 * E);
                IO *e4 = reinterpret_cast<IO *>(&raw);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    e4[e] = (IO)cascade_step<NSEC, ORD, UNIT>(cf, z, (double)e4[e]);
                    if (decltype(capture)::value && zf_owner && c4 * E + e == zf_off % PC) {
#pragma unroll
                        for (int d = 0; d < D; ++d) zf[d] = z[d];
                    }
                }
                *reinterpret_cast<float4 *>(r + c4 * E) = raw;
            }
        };
        auto run_piece = [&](auto capture) __attribute__((always_inline)) {
            run_plane(capture, rr, z0, a.zf);
            asm volatile("" ::: "memory");
            run_plane(capture, ri, z1, a.zf + D);
        };
        if (p == zf_piece) run_piece(std::true_type{});
        else run_piece(std::false_type{});
        __syncthreads();
        int64_t dq_run = 0;
        int dr_run = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = i * kIirThreads + tid;
            const int row = idx >> 3, seg = idx & 7;
            const int64_t g = (row0 + row) * a.T + (int64_t)p * PC + (int64_t)seg * (E / 2);
            IO out[E];
#pragma unroll
            for (int k = 0; k < E / 2; ++k) {
                out[2 * k] = st_re[row * PITCH + seg * (E / 2) + k];
                out[2 * k + 1] = st_im[row * PITCH + seg * (E / 2) + k];
            }
            if (a.dec > 1) {
                // decimating store (see iir_chunk_kernel): a segment holds E / 2 <= 2 <= dec complex samples, so at most
                // one of them is kept
                if (i == 0) {
                    dq_run = g / a.dec;
                    dr_run = (int)(g - dq_run * a.dec);
                }
                const int e0 = dr_run == 0 ? 0 : a.dec - dr_run;
                if (e0 < E / 2 && g + e0 < a.n_keep) {
                    IO re = out[0], im = out[1];
#pragma unroll
                    for (int k = 1; k < E / 2; ++k) {
                        re = (e0 == k) ? out[2 * k] : re;
                        im = (e0 == k) ? out[2 * k + 1] : im;
                    }
                    IO *dst = y + 2 * (dq_run + (dr_run != 0));
                    dst[0] = re;
                    dst[1] = im;
                }
                dq_run += a.dec_dq;
                dr_run += a.dec_dr;
                if (dr_run >= a.dec) { dr_run -= a.dec; ++dq_run; }
            } else if (interior || g + E / 2 <= a.n) {
                *reinterpret_cast<float4 *>(y + 2 * g) = *reinterpret_cast<const float4 *>(out);
            } else if (g < a.n) {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (g + e / 2 < a.n) y[2 * g + e] = out[e];
            }
        }
        __syncthreads();
    }
}

// K2: exclusive scan of W <= 512 workgroup aggregates, one workgroup per batch item:
//   carry[w] = sum_{u<w} (M^256)^(w-1-u) agg[u]
// Hillis-Steele over items with the D x D matvec spread over (item,row) pairs: thread p
// owns row r = p % D of item i = p / D, so one level costs D fma per pair (the matrix
// power for the level and both vector buffers live in LDS).  ~10 us for W = 512, D = 16
// (the first version -- one item per thread, matrix through the scalar cache -- took 78 us).
template <int D>
__global__ __launch_bounds__(1024) void iir_wg_scan_kernel(const double *__restrict__ agg, const double *__restrict__ pw,
                                                           int W, double *__restrict__ carry, const double *__restrict__ zi)
{
    constexpr int kPer = kMaxPairs / 1024;  // (item,row) pairs per thread
    __shared__ double vb[kMaxPairs];
    __shared__ double Ml[D * (D + 1)];  // row pitch D+1: rows land on distinct banks
    const int tid = threadIdx.x;
    const double *in = agg + (size_t)blockIdx.x * W * D;
    double *out = carry + (size_t)blockIdx.x * W * D;
    const int npairs = W * D;
    // items: [zi, agg[0], ..., agg[W-2]]; their inclusive scan IS the carry of workgroups 0..W-1
    for (int p = tid; p < npairs; p += 1024) vb[p] = (p < D) ? (zi ? zi[(size_t)blockIdx.x * D + p] : 0.0) : in[p - D];
    for (int l = 0; l < 10 && (1 << l) < W; ++l) {
        const int s = 1 << l;
        for (int e = tid; e < D * D; e += 1024) Ml[(e / D) * (D + 1) + (e % D)] = pw[(size_t)(8 + l) * D * D + e];
        __syncthreads();
        double nv[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int p = tid + k * 1024;
            double acc = 0.0;
            if (p < npairs) {
                const int i = p / D, r = p - i * D;
                acc = vb[p];
                if (i >= s) {
                    const double *left = &vb[(i - s) * D];
#pragma unroll
                    for (int c = 0; c < D; ++c) acc = fma(Ml[r * (D + 1) + c], left[c], acc);
                }
            }
            nv[k] = acc;
        }
        __syncthreads();  // everyone has read the old values
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int p = tid + k * 1024;
            if (p < npairs) vb[p] = nv[k];
        }
        __syncthreads();
    }
    __syncthreads();
    for (int p = tid; p < npairs; p += 1024) out[p] = vb[p];
}

// ------------------------------------------------------------------ host side
#if SK_SCAN_PART != 2
bool iir_shape_supported(int nsec, int order)
{
    return order == 2 && nsec >= 1 && nsec <= 12;   // (one group: longer cascades are split by the handle)
}

IirHandle::~IirHandle()
{
    if (plan) iir_free(plan);
    if (par) iir_par_free(par);
    for (IirHandle *g : groups) delete g;
    if (group_tmp) (void)hipFree(group_tmp);
    delete twin64;
    if (seq_coef_dev) (void)hipFree(seq_coef_dev);
    if (twin_in) (void)hipFree(twin_in);
    if (twin_out) (void)hipFree(twin_out);
}

void iir_free(IirPlan *p)
{
    if (!p) return;
    if (p->pw_dev) (void)hipFree(p->pw_dev);
    if (p->pwa_dev) (void)hipFree(p->pwa_dev);
    if (p->lb_dev) (void)hipFree(p->lb_dev);
    if (p->lbk_dev) (void)hipFree(p->lbk_dev);
    if (p->gt_dev) (void)hipFree(p->gt_dev);
    if (p->state_dev) (void)hipFree(p->state_dev);
    if (p->v_dev) (void)hipFree(p->v_dev);
    if (p->agg_dev) (void)hipFree(p->agg_dev);
    if (p->lbg_dev) (void)hipFree(p->lbg_dev);
    if (p->ticket_dev) (void)hipFree(p->ticket_dev);
    delete p;
}

// one cascade step on the host (long double) -- used to build the transition matrix
static void host_step(const IirHandle *h, std::vector<long double> &z, long double x)
{
    const int ORD = h->order;
    for (int s = 0; s < h->nsec; ++s) {
        const double *c = h->coef.data() + (size_t)s * (2 * ORD + 1);
        const long double xn = x;
        const long double yv = (long double)c[0] * xn + z[s * ORD];
        for (int k = 1; k < ORD; ++k) z[s * ORD + k - 1] = (long double)c[k] * xn - (long double)c[ORD + k] * yv + z[s * ORD + k];
        z[s * ORD + ORD - 1] = (long double)c[ORD] * xn - (long double)c[2 * ORD] * yv;
        x = yv;
    }
}

static void matmul_ld(const std::vector<long double> &A, const std::vector<long double> &B, std::vector<long double> &C, int D)
{
    std::vector<long double> R((size_t)D * D, 0.0L);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const long double a = A[(size_t)i * D + k];
            if (a == 0.0L) continue;
            for (int j = 0; j < D; ++j) R[(size_t)i * D + j] += a * B[(size_t)k * D + j];
        }
    C.swap(R);
}

static int ensure_plan(IirHandle *h)
{
    if (h->plan) return SKDSP_OK;
    IirPlan *p = new IirPlan();
    p->nsec = h->nsec; p->order = h->order; p->D = h->nsec * h->order;
    const int D = p->D;
    // one-step transition: column i = state after a zero-input step from e_i
    p->A_host.assign((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) {
        std::vector<long double> z(D, 0.0L);
        z[i] = 1.0L;
        host_step(h, z, 0.0L);
        for (int r = 0; r < D; ++r) p->A_host[(size_t)r * D + i] = (double)z[r];
    }
    hipError_t e;
    if ((e = hipMalloc((void **)&p->pw_dev, (size_t)kPowers * D * D * 8)) != hipSuccess ||
        (e = hipMalloc((void **)&p->pwa_dev, (size_t)8 * 4 * 64 * 8)) != hipSuccess ||
        (e = hipMalloc((void **)&p->lb_dev, (size_t)8 * D * D * 8)) != hipSuccess ||
        (e = hipMalloc((void **)&p->lbk_dev, (size_t)32 * D * D * 8)) != hipSuccess ||
        (e = hipMalloc((void **)&p->state_dev, (size_t)4 * D * 8)) != hipSuccess ||
        (e = hipMalloc((void **)&p->agg_dev, (size_t)2 * 2 * kMaxW * D * 8)) != hipSuccess) {
        iir_free(p);
        return hip_fail(e, "hipMalloc(iir plan)", __FILE__, __LINE__);
    }
    h->plan = p;
    return SKDSP_OK;
}

// matrix powers M^(2^l), M = A^T, l = 0..16, for chunk length T (cached)
static int ensure_powers(IirHandle *h, int64_t T, hipStream_t s)
{
    IirPlan *p = h->plan;
    if (p->cached_T == T) return SKDSP_OK;
    const int D = p->D;
    std::vector<long double> base((size_t)D * D), M((size_t)D * D, 0.0L);
    for (size_t i = 0; i < base.size(); ++i) base[i] = p->A_host[i];
    for (int i = 0; i < D; ++i) M[(size_t)i * D + i] = 1.0L;
    // M = A^T by binary exponentiation
    int64_t e = T;
    std::vector<long double> sq = base;
    while (e) {
        if (e & 1) matmul_ld(M, sq, M, D);
        e >>= 1;
        if (e) matmul_ld(sq, sq, sq, D);
    }
    {   // M^k, k = 0..31, transposed so that lane k reads entry (i,j) at [(i*D+j)*32 + k]
        std::vector<long double> Pk((size_t)D * D, 0.0L);
        for (int i = 0; i < D; ++i) Pk[(size_t)i * D + i] = 1.0L;
        std::vector<double> lbk((size_t)32 * D * D);
        for (int k = 0; k < 32; ++k) {
            for (size_t i = 0; i < (size_t)D * D; ++i) lbk[i * 32 + k] = std::isfinite((double)Pk[i]) ? (double)Pk[i] : 0.0;
            matmul_ld(Pk, M, Pk, D);
        }
        SK_HIP(hipMemcpyAsync(p->lbk_dev, lbk.data(), lbk.size() * 8, hipMemcpyHostToDevice, s));
        SK_HIP(hipStreamSynchronize(s));
    }
    p->gt_T = -1;
    if (D <= 32 && (T % kMmPiece == 0 || T == 64 || T == 32)) {
        // G[:, k] = A^(T-1-k) b, b = the state one sample x = 1 leaves behind; stored as the MFMA A operand
        // of step s = k / 4: lane l holds row l & 15, column 4 s + (l >> 4)
        std::vector<long double> g(D, 0.0L);
        host_step(h, g, 1.0L);
        const int NT = D > 16 ? 2 : 1;
        std::vector<double> gt((size_t)NT * T * 16, 0.0);
        for (int64_t k = T - 1; k >= 0; --k) {
            for (int d = 0; d < D; ++d) {
                const long double v = g[d];
                gt[(size_t)(d / 16) * T * 16 + (size_t)(k / 4) * 64 + (size_t)(k % 4) * 16 + (d % 16)] =
                    std::isfinite((double)v) ? (double)v : 0.0;
            }
            host_step(h, g, 0.0L);  // g <- A g
        }
        if (gt.size() * 8 > p->gt_cap) {
            if (p->gt_dev) SK_HIP(hipFree(p->gt_dev));
            p->gt_dev = nullptr; p->gt_cap = 0;
            SK_HIP(hipMalloc((void **)&p->gt_dev, gt.size() * 8));
            p->gt_cap = gt.size() * 8;
        }
        SK_HIP(hipMemcpyAsync(p->gt_dev, gt.data(), gt.size() * 8, hipMemcpyHostToDevice, s));
        SK_HIP(hipStreamSynchronize(s));
        p->gt_T = T;
    }
    // A transition power counts as vanished when its largest entry is below `negl`: 1e-30 for float64 signals (nothing a
    // float64 recurrence could resolve), 1e-18 for float32 signals (the dropped term is under a tenth of an ulp of the
    // float64 STATE it would be added to, and eleven orders below the float32 rounding of the output) -- for the config-4
    // cascade (pole radius 0.99465) that is 60 chunks of 128 samples instead of 101: one scan level less.
    const long double negl = dtype_double(h->dtype) ? 1e-30L : 1e-18L;
    std::vector<double> pw((size_t)kPowers * D * D);
    p->n_lv = kPowers;
    for (int l = 0; l < kPowers; ++l) {
        long double mx = 0.0L;
        for (auto v : M) mx = fabsl(v) > mx ? fabsl(v) : mx;
        if (std::isfinite((double)mx) && mx < negl && l < p->n_lv) p->n_lv = l;
        for (size_t i = 0; i < (size_t)D * D; ++i) {
            long double v = M[i];
            if (!std::isfinite((double)v)) v = 0.0L;  // unstable filter overflow: the reference overflows too
            pw[(size_t)l * D * D + i] = (double)v;
        }
        if (l + 1 < kPowers) matmul_ld(M, M, M, D);
    }
    // carry look-back: (M^256)^k until every entry is below 1e-30 (its contribution is then far
    // under one ulp of anything the float64 recurrence itself could resolve)
    {
        std::vector<long double> Mw((size_t)D * D), Pk;
        for (size_t i = 0; i < (size_t)D * D; ++i) Mw[i] = pw[(size_t)8 * D * D + i];
        Pk = Mw;
        std::vector<double> lb((size_t)8 * D * D, 0.0);
        p->n_lb = 0;
        for (int k = 1; k <= 8; ++k) {  // Pk = Mw^k
            long double mx = 0.0L;
            for (auto v : Pk) mx = fabsl(v) > mx ? fabsl(v) : mx;
            if (!(mx >= negl)) { p->n_lb = k; break; }  // terms k.. are negligible: keep k terms (0..k-1)
            if (k == 8) break;
            for (size_t i = 0; i < (size_t)D * D; ++i) lb[(size_t)(k - 1) * D * D + i] = (double)Pk[i];
            matmul_ld(Pk, Mw, Pk, D);
        }
        SK_HIP(hipMemcpyAsync(p->lb_dev, lb.data(), lb.size() * 8, hipMemcpyHostToDevice, s));
        SK_HIP(hipStreamSynchronize(s));
    }
    SK_HIP(hipMemcpyAsync(p->pw_dev, pw.data(), pw.size() * 8, hipMemcpyHostToDevice, s));
    std::vector<double> pwa((size_t)8 * 4 * 64, 0.0);
    if (D <= 16) {  // the same powers as A operands of v_mfma_f64_16x16x4: step r of level l, lane t: M_l[t & 15][4 r + (t >> 4)]
        for (int l = 0; l < 8; ++l)
            for (int r = 0; r < 4; ++r)
                for (int t = 0; t < 64; ++t) {
                    const int row = t & 15, col = 4 * r + (t >> 4);
                    if (row < D && col < D) pwa[((size_t)l * 4 + r) * 64 + t] = pw[(size_t)l * D * D + (size_t)row * D + col];
                }
    }
    SK_HIP(hipMemcpyAsync(p->pwa_dev, pwa.data(), pwa.size() * 8, hipMemcpyHostToDevice, s));
    SK_HIP(hipStreamSynchronize(s));  // pw / pwa are stack-lifetime host buffers
    p->cached_T = T;
    return SKDSP_OK;
}

#endif  // SK_SCAN_PART != 2

template <int NSEC, int ORD, typename IO>
static int launch_shape(IirHandle *h, IirArgs &a, int nbatch, int W, hipStream_t s)
{
    constexpr int D = NSEC * ORD;
    Coef<NSEC, ORD> cf;
    std::memcpy(cf.c, h->coef.data(), sizeof(cf.c));
    IirPlan *p = h->plan;
    double *agg = p->agg_dev;
    double *carry = p->agg_dev + (size_t)2 * kMaxW * D;
    a.agg = agg;
    a.carry = carry;
    a.lbmat = p->lb_dev;
    a.n_lb = p->n_lb;
    a.n_lv = p->n_lv < 8 ? p->n_lv : 8;
    // aggregate-free mode: matrix-pipe K1, carries from the chunk states themselves, unchanged K3
    const bool fast = p->n_lv <= 5 && D <= 32 && ORD == 2 && a.T % kMmPiece == 0 && p->gt_T == a.T && !opt().iir_no_mfma;
    if (a.il) {
        if (!fast || a.T % 64 != 0) return 1;  // not applicable (error codes are negative): the caller takes the planar detour
        const int64_t waves = (a.J + 15) / 16;
        if (D <= 16)
            hipLaunchKernelGGL((iir_k1c_mfma_kernel<IO, 1>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const IO *)a.x, a.n, a.T,
                               a.J, (const double *)p->gt_dev, a.v, D);
        else
            hipLaunchKernelGGL((iir_k1c_mfma_kernel<IO, 2>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const IO *)a.x, a.n, a.T,
                               a.J, (const double *)p->gt_dev, a.v, D);
        SK_HIP(hipGetLastError());
        hipLaunchKernelGGL((iir_carry_kernel<D, ORD>), dim3(W, 2), dim3(256), 0, s, (const double *)a.v, (const double *)p->lbk_dev, a.J,
                           a.zi, carry);
        a.n_lb = 0;
        if (NSEC >= 2 && h->unit_tail) hipLaunchKernelGGL((iir_k3c_kernel<NSEC, ORD, IO, (NSEC >= 2)>), dim3(W), dim3(kIirThreads), 0, s, a, cf);
        else hipLaunchKernelGGL((iir_k3c_kernel<NSEC, ORD, IO>), dim3(W), dim3(kIirThreads), 0, s, a, cf);
        SK_HIP(hipGetLastError());
        return SKDSP_OK;
    }
    if (fast) {
        const int64_t waves = (a.J + 15) / 16;
        const bool no_k1r = false;
        const int np = (int)(a.T / kMmPiece);
        if (D <= 16 && !no_k1r && (np == 1 || np == 2 || np == 4) && a.T == (int64_t)np * kMmPiece) {
            // G in registers: persistent workgroups (3 per CU), each iteration 4 / np groups of 16 chunks
            const int64_t ngroups = waves, per_wg = 4 / np;
            const int wgs_per_cu = 2;
            const unsigned grid = (unsigned)std::min<int64_t>((ngroups + per_wg - 1) / per_wg, (int64_t)wgs_per_cu * ctx().num_cus);
#define SK_K1R(NP) hipLaunchKernelGGL((iir_k1r_kernel<IO, NP>), dim3(grid, nbatch), dim3(256), 0, s, (const IO *)a.x, a.n, a.J, a.batch_stride, (const double *)p->gt_dev, a.v, D)
            if (np == 1) SK_K1R(1);
            else if (np == 2) SK_K1R(2);
            else SK_K1R(4);
#undef SK_K1R
        } else if (D <= 16)
            hipLaunchKernelGGL((iir_k1_mfma_kernel<IO, 1>), dim3((unsigned)((waves + 3) / 4), nbatch), dim3(256), 0, s, (const IO *)a.x,
                               a.n, a.T, a.J, a.batch_stride, (const double *)p->gt_dev, a.v, D);
        else
            hipLaunchKernelGGL((iir_k1_mfma_kernel<IO, 2>), dim3((unsigned)((waves + 3) / 4), nbatch), dim3(256), 0, s, (const IO *)a.x,
                               a.n, a.T, a.J, a.batch_stride, (const double *)p->gt_dev, a.v, D);
        SK_HIP(hipGetLastError());
        hipLaunchKernelGGL((iir_carry_kernel<D, ORD>), dim3(W, nbatch), dim3(256), 0, s, (const double *)a.v, (const double *)p->lbk_dev,
                           a.J, a.zi, carry);
        a.n_lb = 0;  // K3 reads the carries
    } else {
        hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, false>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    }
    SK_HIP(hipGetLastError());
    if (p->n_lb == 0 && !fast) {  // slowly decaying / marginally stable filter: full scan of the workgroup aggregates
        hipLaunchKernelGGL((iir_wg_scan_kernel<D>), dim3(nbatch), dim3(1024), 0, s, (const double *)agg, (const double *)p->pw_dev, W, carry, a.zi);
        SK_HIP(hipGetLastError());
    }
    if (NSEC >= 2 && h->unit_tail) hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, true, (NSEC >= 2)>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    else hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, true>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

template <typename IO>
static int dispatch_shape(IirHandle *h, IirArgs &a, int nbatch, int W, hipStream_t s)
{
#define SK_SOS(N) case N: return launch_shape<N, 2, IO>(h, a, nbatch, W, s);
    if (h->order == 2) {
        switch (h->nsec) {
            SK_SOS(1) SK_SOS(2) SK_SOS(3) SK_SOS(4) SK_SOS(5) SK_SOS(6) SK_SOS(7) SK_SOS(8) SK_SOS(9) SK_SOS(10) SK_SOS(11) SK_SOS(12)
        }
    }
#undef SK_SOS
    SK_CHECK(false, SKDSP_ERR_UNSUPPORTED, "iir: unsupported cascade shape (%d sections of order %d)", h->nsec, h->order);
}

// the float64 half of the dispatch lives in its own object (SK_SCAN_PART)
int iir_dispatch_shape_f64(IirHandle *h, IirArgs &a, int nbatch, int W, hipStream_t s);
#if SK_SCAN_PART != 1
int iir_dispatch_shape_f64(IirHandle *h, IirArgs &a, int nbatch, int W, hipStream_t s) { return dispatch_shape<double>(h, a, nbatch, W, s); }
#endif

#if SK_SCAN_PART != 2
// x_dev/y_dev: real planar arrays (float or double per h->dtype's precision); complex
// callers deinterleave first (iir_api.hip) and pass nbatch = 2 with batch_stride.
int iir_launch_planar(IirHandle *h, const void *x, int64_t n, int nbatch, int64_t batch_stride, void *y, hipStream_t s,
                      const double *zi_host, double *zf_host, int interleaved, int dec)
{
    if (n <= 0) {
        if (zf_host) {
            if (zi_host) memcpy(zf_host, zi_host, (size_t)nbatch * h->nsec * h->order * 8);
            else memset(zf_host, 0, (size_t)nbatch * h->nsec * h->order * 8);
        }
        return SKDSP_OK;
    }
    if (h->seq) {   // an ill-conditioned cascade: the reference's own recursion (iir_seq.hip)
        if (interleaved) return 1;
        return iir_seq_launch(h, x, n, nbatch, batch_stride, batch_stride, y, s, zi_host, zf_host, dec);
    }
    if (h->twin64) {
        // the float64 detour (see IirHandle::twin64): planar float32 in, planar float32 out
        if (interleaved) return 1;
        const int64_t tot = nbatch > 1 ? batch_stride * nbatch : n;
        auto grow = [&](void *&p, size_t &have, size_t need) -> int {
            if (need <= have) return SKDSP_OK;
            if (p) {
                SK_HIP(hipStreamSynchronize(s));
                SK_HIP(hipFree(p));
                p = nullptr; have = 0;
            }
            SK_HIP(hipMalloc(&p, need));
            have = need;
            return SKDSP_OK;
        };
        int rc = grow(h->twin_in, h->twin_in_bytes, (size_t)tot * 8 + 256);
        if (rc) return rc;
        if ((rc = convert_launch(x, h->twin_in, tot, true, s))) return rc;
        void *o64 = h->twin_in;
        int64_t out_tot = tot;
        if (dec > 1) {   // (one real row: the kept outputs go to a buffer of their own)
            out_tot = n / dec;
            if ((rc = grow(h->twin_out, h->twin_out_bytes, (size_t)out_tot * 8 + 256))) return rc;
            o64 = h->twin_out;
        }
        if ((rc = iir_launch_planar(h->twin64, h->twin_in, n, nbatch, batch_stride, o64, s, zi_host, zf_host, 0, dec))) return rc;
        return convert_launch(o64, y, out_tot, false, s);
    }
    if (!h->groups.empty()) {
        // consecutive groups of sections, each through this function: group 0 reads x, the others filter y in place; a decimating call keeps
        // the full-rate signal of all groups but the last in a buffer of the handle; the states are per section, so a group takes its slice
        if (interleaved) return 1;   // (the caller's planar form splits; an interleaved group chain could stop half-way through "not applicable")
        const int D = h->nsec * 2;
        const size_t esz = dtype_double(h->dtype) ? 8 : 4;
        void *mid = y;
        if (dec > 1) {
            const size_t need = (size_t)(nbatch > 1 ? batch_stride * nbatch : n) * esz + 256;
            if (need > h->group_tmp_bytes) {
                if (h->group_tmp) {
                    SK_HIP(hipStreamSynchronize(s));
                    SK_HIP(hipFree(h->group_tmp));
                    h->group_tmp = nullptr; h->group_tmp_bytes = 0;
                }
                SK_HIP(hipMalloc(&h->group_tmp, need));
                h->group_tmp_bytes = need;
            }
            mid = h->group_tmp;
        }
        std::vector<double> zi_g, zf_g;
        for (size_t gi = 0; gi < h->groups.size(); ++gi) {
            IirHandle *g = h->groups[gi];
            const bool last = gi + 1 == h->groups.size();
            const int Dg = g->nsec * 2;
            const double *zi_p = nullptr;
            double *zf_p = nullptr;
            if (zi_host) {
                zi_g.resize((size_t)nbatch * Dg);
                for (int b = 0; b < nbatch; ++b) memcpy(zi_g.data() + (size_t)b * Dg, zi_host + (size_t)b * D + 2 * g->group_first, (size_t)Dg * 8);
                zi_p = zi_g.data();
            }
            if (zf_host) {
                zf_g.assign((size_t)nbatch * Dg, 0.0);
                zf_p = zf_g.data();
            }
            const int rc = iir_launch_planar(g, gi == 0 ? x : mid, n, nbatch, batch_stride, last ? y : mid, s, zi_p, zf_p, 0, last ? dec : 1);
            if (rc) return rc;
            if (zf_host)
                for (int b = 0; b < nbatch; ++b) memcpy(zf_host + (size_t)b * D + 2 * g->group_first, zf_g.data() + (size_t)b * Dg, (size_t)Dg * 8);
        }
        return SKDSP_OK;
    }
    // Parallel form (iir_par.hip): the same transfer function as independent two-state branches, every wave its own segment.
    // No state crosses these calls (scipy's zi / zf live in the cascade's coordinates: such calls keep the kernels below).
    if (zi_host == nullptr && zf_host == nullptr && opt().iir_par > 0 && h->order == 2 && h->nsec <= 8 &&
        (interleaved || dec <= 1 || nbatch == 1)) {
        // (interleaved complex: re and im are two independent real signals on one memory stream: lanes alternate between them;
        // with dec > 1 only where a segment's kept outputs fit the wave's stage image -- else 1 comes back)
        const int r = interleaved ? iir_par_launch(h, x, n, 1, 0, 0, y, s, dec, 1)
                                  : iir_par_launch(h, x, n, nbatch, batch_stride, batch_stride, y, s, dec);
        if (r != 1) return r;   // (1 = not applicable: poles shared between sections, slow decay, ...)
    }
    int rc = ensure_plan(h);
    if (rc) return rc;
    IirPlan *p = h->plan;
    const int D = p->D;
    // Single-pass scan (one launch, x read once): real signals, <= 8 biquads whose transition over one 256-chunk segment
    // is below 1e-30 (n_lb == 1 for the segment's chunk length), enough segments to fill the chip.
    bool fused = false;
    {
        // chunk length: 128 float32 / 64 float64 samples (real), 64 complex64 / 32 complex128 samples (interleaved)
        const int64_t Tf = (dtype_double(h->dtype) ? 64 : 128) / (interleaved ? 2 : 1);
        int &fstate = interleaved ? p->fused_state_c : p->fused_state;   // applicability only (cached); the policy is per call
        int &fnlv = interleaved ? p->fused_nlv_c : p->fused_nlv;
        const bool wanted = h->order == 2 && D <= 16 && opt().iir_two_pass <= 0 && fstate >= 0 &&
                            (dec <= 1 || ((nbatch == 1 || interleaved) && zf_host == nullptr)) &&
                            n >= Tf * kIirThreads * (int64_t)ctx().num_cus;
        if (wanted && fstate == 0) {
            rc = ensure_powers(h, Tf, s);
            if (rc) return rc;
            fstate = (p->n_lb == 1 && p->gt_T == Tf) ? 1 : -1;
            fnlv = p->n_lv;
        }
        if (wanted && fstate == 1) {
            // Real signals: the single pass wins or ties everywhere it applies (tools/ab_iir.py, 2^26, same box): low-pass designs
            // 0.11-0.13 vs 0.15 ms, float64 0.19-0.28 vs 0.36-0.42 ms; the 8-biquad elliptic band-pass of BASELINE config 4
            // (6 scan levels of a 16 x 16 transition per 128-sample chunk) 0.175 vs 0.184 ms since its scan runs on the
            // matrix pipe (iir_fused.hip: 0.197 ms with the per-thread VALU scan) -- and it moves 8 instead of 12 bytes per sample.
            // interleaved complex64 (two scans per 64-sample chunk): 0.22-0.29 vs 0.42-0.45 ms for low-pass designs (<= 4
            // levels), 0.56 vs 0.46 ms for the config-4 cascade (7 levels): those stay two-pass unless iir_two_pass = -1
            fused = !(interleaved && !dtype_double(h->dtype) && fnlv >= 6 && opt().iir_two_pass >= 0);
            if (fused) {
                rc = ensure_powers(h, Tf, s);   // (a no-op unless a two-pass call re-made the tables for its chunk length)
                if (rc) return rc;
            }
        }
    }
    int maxW = kMaxPairs / D;
    if (maxW > kMaxW) maxW = kMaxW;
    const int64_t maxChunks = (int64_t)maxW * kIirThreads;
    int64_t T = (n + maxChunks - 1) / maxChunks;
    T = ((T + kPiece - 1) / kPiece) * kPiece;
    if (T < kPiece) T = kPiece;
    if (T >= kMmPiece) T = ((T + kMmPiece - 1) / kMmPiece) * kMmPiece;  // whole 128-sample pieces for the matrix-pipe K1
    const int64_t J = (n + T - 1) / T;
    const int W = (int)((J + kIirThreads - 1) / kIirThreads);
    if (!fused) {
        rc = ensure_powers(h, T, s);
        if (rc) return rc;
    }
    const size_t need = fused ? 0 : (size_t)nbatch * D * J * 8;
    if (need > p->v_cap) {
        if (p->v_dev) SK_HIP(hipFree(p->v_dev));
        p->v_dev = nullptr; p->v_cap = 0;
        SK_HIP(hipMalloc((void **)&p->v_dev, need));
        p->v_cap = need;
    }
    IirArgs a;
    a.x = x; a.y = y; a.n = n; a.T = T; a.J = J; a.batch_stride = batch_stride;
    a.il = interleaved ? 1 : 0;
    a.pw = p->pw_dev; a.v = p->v_dev; a.agg = nullptr; a.carry = nullptr; a.lbmat = nullptr; a.n_lb = 0; a.n_lv = 8;
    a.zi = nullptr; a.zf = nullptr;
    a.dec = dec > 1 ? dec : 1;
    a.n_keep = (n / a.dec) * a.dec;
    {
        // rows between a thread's staged segments x T (the interleaved complex kernel stages 8 segments per row piece)
        const int64_t step = (interleaved ? kIirThreads / 8 : kIirThreads / (kPiece / (16 / (dtype_double(h->dtype) ? 8 : 4)))) * T;
        a.dec_dq = (int)(step / a.dec);
        a.dec_dr = (int)(step % a.dec);
    }
    SK_CHECK(a.dec == 1 || (zf_host == nullptr && (interleaved || nbatch == 1)), SKDSP_ERR_UNSUPPORTED,
             "iir: decimating store needs a real or interleaved complex signal and no state output");
    std::vector<double> zi_int;  // the caller's DF2T states in the internal factorisation (IirHandle::state_scale)
    if (zi_host) {
        if (!h->state_scale.empty()) {
            zi_int.resize((size_t)nbatch * D);
            for (int b = 0; b < nbatch; ++b)
                for (int d = 0; d < D; ++d) zi_int[(size_t)b * D + d] = zi_host[(size_t)b * D + d] * h->state_scale[d];
            zi_host = zi_int.data();
        }
        SK_HIP(hipMemcpyAsync(p->state_dev, zi_host, (size_t)nbatch * D * 8, hipMemcpyHostToDevice, s));
        if (!zi_int.empty()) SK_HIP(hipStreamSynchronize(s));  // zi_int is a local
        a.zi = p->state_dev;
    }
    if (zf_host) a.zf = p->state_dev + 2 * D;
    SK_CHECK(nbatch >= 1 && nbatch <= 2, SKDSP_ERR_BADARG, "iir: batch must be 1 or 2");
    if (fused) {
        rc = iir_fused_launch(h, x, n, nbatch, batch_stride, y, a.zi, a.zf, s, dec, interleaved);
    } else {
        rc = dtype_double(h->dtype) ? iir_dispatch_shape_f64(h, a, nbatch, W, s) : dispatch_shape<float>(h, a, nbatch, W, s);
    }
    if (rc) return rc;  // (1 = interleaved path not applicable, nothing was launched)
    if (!fused) note_path("iir_scan");   // (recorded once the two-pass kernels WERE launched: iir_seq, the twin, the groups, iir_par and iir_fused note themselves)
    if (zf_host) {
        SK_HIP(hipMemcpyAsync(zf_host, p->state_dev + 2 * D, (size_t)nbatch * D * 8, hipMemcpyDeviceToHost, s));
        SK_HIP(hipStreamSynchronize(s));
        if (!h->state_scale.empty())
            for (int b = 0; b < nbatch; ++b)
                for (int d = 0; d < D; ++d) zf_host[(size_t)b * D + d] /= h->state_scale[d];
    }
    return SKDSP_OK;
}

#endif  // SK_SCAN_PART != 2

}  // namespace skdsp
