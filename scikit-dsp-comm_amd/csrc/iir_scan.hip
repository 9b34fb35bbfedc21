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
// piece) compile side by side: 1 = the float32 kernels and their launch (build/iir_scan.o), 2 = the float64 ones
// (build/iir_scan_f64.o); 0 = everything in one object (variant builds).  There is no host code here but the launch.
#ifndef SK_SCAN_PART
#define SK_SCAN_PART 0
#endif

namespace skdsp {

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
static_assert(kMmPiece == 128, "the staging below is laid out for 128-sample pieces (iir_scan_plan.hpp: kMmPiece)");
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

// ------------------------------------------------------------------ launch
// The two-pass sequence for finished arguments and a decided form (iir_common.hpp: ScanLaunch; the decision is iir_route.hpp, the plan and
// the arguments are made by iir_api.hip).  What is asked for must be what the rules of iir_scan_plan.hpp allow.
template <int NSEC, int ORD, typename IO>
static int launch_shape(const ScanLaunch &L, IirArgs &a, hipStream_t s)
{
    constexpr int D = NSEC * ORD;
    Coef<NSEC, ORD> cf;
    std::memcpy(cf.c, L.coef, sizeof(cf.c));
    const int nbatch = L.nbatch, W = L.W;
    const bool fast = L.form.fast, unit = NSEC >= 2 && L.form.unit_tail;
    const ScanFacts facts{L.n_lv, a.n_lb, L.gt_T};
    SK_CHECK(L.form.k1 == scan_k1(fast, a.il != 0, D, a.T) && (!fast || scan_fast(facts, D, ORD, a.T, 0)) &&
                 (!a.il || (nbatch == 2 && scan_interleaved_applies(fast, a.T))),
             SKDSP_ERR_UNSUPPORTED, "iir_scan: the two-pass kernels asked for do not take this call (%d sections, chunks of %lld)", NSEC, (long long)a.T);
    const int64_t waves = (a.J + 15) / 16;
    if (a.il) {
        if (D <= 16)
            hipLaunchKernelGGL((iir_k1c_mfma_kernel<IO, 1>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const IO *)a.x, a.n, a.T,
                               a.J, L.gt, a.v, D);
        else
            hipLaunchKernelGGL((iir_k1c_mfma_kernel<IO, 2>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const IO *)a.x, a.n, a.T,
                               a.J, L.gt, a.v, D);
        SK_HIP(hipGetLastError());
        hipLaunchKernelGGL((iir_carry_kernel<D, ORD>), dim3(W, 2), dim3(256), 0, s, (const double *)a.v, L.lbk, a.J, a.zi, (double *)a.carry);
        if (unit) hipLaunchKernelGGL((iir_k3c_kernel<NSEC, ORD, IO, (NSEC >= 2)>), dim3(W), dim3(kIirThreads), 0, s, a, cf);
        else hipLaunchKernelGGL((iir_k3c_kernel<NSEC, ORD, IO>), dim3(W), dim3(kIirThreads), 0, s, a, cf);
        SK_HIP(hipGetLastError());
        return SKDSP_OK;
    }
    if (fast) {
        if (L.form.k1 == kK1Regs) {
            // G in registers: persistent workgroups (2 per CU), each iteration 4 / np groups of 16 chunks
            const int np = (int)(a.T / kMmPiece);
            const int64_t ngroups = waves, per_wg = 4 / np;
            const int wgs_per_cu = 2;
            const unsigned grid = (unsigned)std::min<int64_t>((ngroups + per_wg - 1) / per_wg, (int64_t)wgs_per_cu * L.num_cus);
#define SK_K1R(NP) hipLaunchKernelGGL((iir_k1r_kernel<IO, NP>), dim3(grid, nbatch), dim3(256), 0, s, (const IO *)a.x, a.n, a.J, a.batch_stride, L.gt, a.v, D)
            if (np == 1) SK_K1R(1);
            else if (np == 2) SK_K1R(2);
            else SK_K1R(4);
#undef SK_K1R
        } else if (D <= 16)
            hipLaunchKernelGGL((iir_k1_mfma_kernel<IO, 1>), dim3((unsigned)((waves + 3) / 4), nbatch), dim3(256), 0, s, (const IO *)a.x,
                               a.n, a.T, a.J, a.batch_stride, L.gt, a.v, D);
        else
            hipLaunchKernelGGL((iir_k1_mfma_kernel<IO, 2>), dim3((unsigned)((waves + 3) / 4), nbatch), dim3(256), 0, s, (const IO *)a.x,
                               a.n, a.T, a.J, a.batch_stride, L.gt, a.v, D);
        SK_HIP(hipGetLastError());
        hipLaunchKernelGGL((iir_carry_kernel<D, ORD>), dim3(W, nbatch), dim3(256), 0, s, (const double *)a.v, L.lbk, a.J, a.zi, (double *)a.carry);
    } else {
        hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, false>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    }
    SK_HIP(hipGetLastError());
    if (a.n_lb == 0 && !fast) {  // slowly decaying / marginally stable filter: full scan of the workgroup aggregates
        hipLaunchKernelGGL((iir_wg_scan_kernel<D>), dim3(nbatch), dim3(1024), 0, s, (const double *)a.agg, a.pw, W, (double *)a.carry, a.zi);
        SK_HIP(hipGetLastError());
    }
    if (unit) hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, true, (NSEC >= 2)>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    else hipLaunchKernelGGL((iir_chunk_kernel<NSEC, ORD, IO, true>), dim3(W, nbatch), dim3(kIirThreads), 0, s, a, cf);
    SK_HIP(hipGetLastError());
    return SKDSP_OK;
}

template <typename IO>
static int dispatch_shape(const ScanLaunch &L, IirArgs &a, hipStream_t s)
{
#define SK_SOS(N) case N: return launch_shape<N, 2, IO>(L, a, s);
    if (L.order == 2) {
        switch (L.nsec) {
            SK_SOS(1) SK_SOS(2) SK_SOS(3) SK_SOS(4) SK_SOS(5) SK_SOS(6) SK_SOS(7) SK_SOS(8) SK_SOS(9) SK_SOS(10) SK_SOS(11) SK_SOS(12)
        }
    }
#undef SK_SOS
    SK_CHECK(false, SKDSP_ERR_UNSUPPORTED, "iir: unsupported cascade shape (%d sections of order %d)", L.nsec, L.order);
}

// each precision's kernels live in an object of their own (SK_SCAN_PART): what this object instantiates
#if SK_SCAN_PART == 0 || SK_SCAN_PART == 1
int iir_scan_launch_f32(const ScanLaunch &L, IirArgs &a, hipStream_t s) { return dispatch_shape<float>(L, a, s); }
#endif
#if SK_SCAN_PART == 0 || SK_SCAN_PART == 2
int iir_scan_launch_f64(const ScanLaunch &L, IirArgs &a, hipStream_t s) { return dispatch_shape<double>(L, a, s); }
#endif

}  // namespace skdsp
