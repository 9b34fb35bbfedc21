/*
 * skdsp.h -- C ABI of libskdsp_hip.so: the MI355X (gfx950) replacement for the
 * native kernels that scikit-dsp-comm's streaming-filter hot path executes.
 *
 * The reference has NO FFI of its own for this path: it is pure Python whose
 * arithmetic is one-line calls into scipy.signal / numpy.  The entry points
 * below are therefore "what a binding for this path would bind": one entry per
 * reference call site, cited as /root/reference/src/sk_dsp_comm/<file>:<line>.
 * INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success or a negative skdsp_status; the
 *     message for the calling thread is in skdsp_last_error().
 *   - dtype = arithmetic/storage type of the signal: F32/C64 (hot path),
 *     F64/C128 (direct-form kernels in double, for float64 callers).
 *     Complex is interleaved (re,im), C-contiguous, as NumPy stores it.
 *   - coefficient arrays are always host float64 / complex128 (what the
 *     reference objects hold); the library rounds once to the signal dtype.
 *   - "*_dev" variants take DEVICE pointers (from skdsp_malloc) and run
 *     asynchronously on the library stream; host variants copy in/out and
 *     return after the stream is idle.  The caller owns every buffer; the
 *     library copies coefficients at create() and never retains x/y.
 *   - n_hist: number of valid samples stored immediately BEFORE x_dev[0] in the
 *     same allocation (x_dev[-n_hist..-1]).  0 = zero initial state, which is
 *     what every reference call uses (lfilter/sosfilt without zi).  The sharded
 *     path uses it for the Ntaps-1 halo received from the left neighbour.
 *   - a "*_dev" call reads x_dev[-n_hist .. n-1] and nothing else (n_hist = 0 where the entry point takes none; one such
 *     window per row for the rows forms): whatever lies in front of or behind it in the allocation changes no output bit.
 *   - a handle serialises its own calls.  Calls lock the SLOT they run on (a slot = one GPU binding with its stream
 *     and workspaces): caller threads all use slot 0, so their calls take turns on its stream; the worker threads of
 *     a multi-slot host call run concurrently, one per slot.  ctypes releases the GIL around each call.
 */
#ifndef SKDSP_H
#define SKDSP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { SKDSP_F32 = 0, SKDSP_C64 = 1, SKDSP_F64 = 2, SKDSP_C128 = 3 } skdsp_dtype;

typedef enum {
    SKDSP_OK = 0,
    SKDSP_ERR_BADARG = -1,   /* -> ValueError / TypeError in the Python mirror */
    SKDSP_ERR_NODEVICE = -2, /* no HIP device: the product path fails loudly   */
    SKDSP_ERR_NOMEM = -3,
    SKDSP_ERR_HIP = -4,
    SKDSP_ERR_RCCL = -5,
    SKDSP_ERR_UNSUPPORTED = -6
} skdsp_status;

/* FIR algorithm selector (skdsp_fir_set_algo). AUTO picks by dtype / tap count. */
typedef enum { SKDSP_FIR_AUTO = 0, SKDSP_FIR_DIRECT = 1, SKDSP_FIR_OLS = 2 } skdsp_fir_algo;

typedef void *skdsp_handle;

/* ---- runtime ------------------------------------------------------------ */
int skdsp_init(int device);               /* bind the caller's slot (slot 0) to one GPU, create its stream */
/* Bind slots 0 .. ndev-1 to the listed GPUs (slot 0 = the device every *_dev entry point and handle uses).  With more
 * than one slot bound, the host-pointer FIR entry points deal the chunks of a long vector to all of them, one worker
 * thread, stream and PCIe link each (the reference's single call multirate_FIR(b).filter(x), multirate_helper.py:104-109,
 * then scales over the node without a launcher).  A device may be listed more than once. */
int skdsp_init_devices(const int *devices, int ndev);
int skdsp_slot_count(void);
int skdsp_shutdown(void);
int skdsp_device_count(void);
int skdsp_device_info(char *name, int name_cap, int *compute_units, int64_t *hbm_bytes, int *clock_khz);
const char *skdsp_last_error(void);
/* Test / diagnostic aid (no reference counterpart): the comma-joined names of the kernels families the calling thread's API calls have
 * launched since the last clear ("fir_ols", "fir_bx", "fir_up4k", "iir_par", ...), so that a parity test can assert that a shape
 * reaches the engine it means to exercise.  clear != 0 empties the record. */
int skdsp_debug_path(char *buf, int cap, int clear);
const char *skdsp_version(void);
/* Run-time switches (algorithm A/B selectors, pipeline chunk size, ...).  Each option NAME is read once from the
 * environment variable SKDSP_<NAME> when the library first needs it; afterwards only these calls change it, so no
 * launch path calls getenv().  Names: see struct Options in csrc/skdsp_internal.hpp.  Unknown name -> BADARG. */
int skdsp_set_option(const char *name, int value);
int skdsp_get_option(const char *name, int *value);

int skdsp_malloc(void **dptr, int64_t bytes);
int skdsp_free(void *dptr);
/* Page-locked host memory.  A copy back into a FRESH pageable array (np.empty) runs at ~25-30 GB/s on this platform
 * (page population + first device access), into page-locked memory at the link rate (56 GB/s): the Python layer hands
 * out result arrays backed by recycled blocks from here. */
int skdsp_host_alloc(void **hptr, int64_t bytes);
int skdsp_host_free(void *hptr);
int skdsp_memcpy_h2d(void *dst_dev, const void *src_host, int64_t bytes);
int skdsp_memcpy_d2h(void *dst_host, const void *src_dev, int64_t bytes);
int skdsp_memcpy_d2d(void *dst_dev, const void *src_dev, int64_t bytes);
int skdsp_memset(void *dst_dev, int value, int64_t bytes);
int skdsp_sync(void);                      /* wait for the library stream */
/* HIP-event stopwatch on the library stream (bench.py times kernels with it) */
int skdsp_timer_start(void);
int skdsp_timer_stop(float *elapsed_ms);   /* synchronises on the stop event */
/* what the last skdsp_timer_stop of the calling thread's slot measured, in ms (SURVEY.md 8(b)'s name for it); -1 before the first */
double skdsp_last_kernel_ms(void);
/* fill a device buffer with counter-based N(0,1)/sqrt(2) complex (or N(0,1) real)
 * noise keyed by (seed, global sample index): any window can be regenerated. */
int skdsp_fill_noise_dev(void *x_dev, int64_t n, int dtype, uint64_t seed, int64_t first_index);

/* ---- FIR: multirate_FIR (multirate_helper.py:95-127) ---------------------- */
/* ctor, multirate_helper.py:95-101.  taps: ntaps float64 (taps_complex=0) or
 * ntaps complex128 (taps_complex=1). */
int skdsp_fir_create(const void *taps, int ntaps, int taps_complex, int dtype, skdsp_handle *out);
int skdsp_fir_set_algo(skdsp_handle h, int algo);
int skdsp_fir_get_algo(skdsp_handle h, int64_t n, int *algo_used);
/* .filter(x): signal.lfilter(b,[1],x), multirate_helper.py:104-109.  y has n samples. */
int skdsp_fir_filter(skdsp_handle h, const void *x, int64_t n, void *y);
int skdsp_fir_filter_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev);
/* The same call spread over the GPUs of one process (SURVEY 8(b) / BASELINE config 5 without a launcher): the host vector is cut into
 * contiguous sample blocks, one range of chunks per slot bound by skdsp_init_devices, each chunk staged with the Ntaps-1 samples in
 * front of it -- the halo comes from the caller's array, so the GPUs exchange nothing.  ngpu: slots to use, 0 = all bound
 * (skdsp_fir_filter uses all of them as well; this entry lets a caller choose).  Device-resident shards with an RCCL halo
 * between processes: skdsp_fir_filter_shard_dev below. */
int skdsp_fir_filter_sharded(skdsp_handle h, const void *x, int64_t n, void *y, int ngpu);
/* N-D inputs: lfilter filters along the last axis in ONE call (multirate_helper.py:108).  nrow rows of n samples, each
 * filtered from rest: one pitched copy in, one launch over the rows laid end to end with Ntaps-1 zeros between them,
 * one pitched copy out (host form: rows contiguous; device form: x_stride / y_stride elements between rows, >= n). */
int skdsp_fir_filter_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, void *y);
int skdsp_fir_filter_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev);
/* .up(x,L): lfilter(b,[1], L*upsample(x,L)), multirate_helper.py:112-118.  y has n*L samples. */
int skdsp_fir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y);
int skdsp_fir_up_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev);
/* .dn(x,M): downsample(lfilter(b,[1],x), M), multirate_helper.py:121-127.  y has n/M samples. */
int skdsp_fir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y);
int skdsp_fir_dn_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev);
/* fused rational resampler = downsample(.up(x,L), M) (BASELINE.json config 3;
 * sigsys.py:3078-3083 applied to multirate_helper.py:112-118).  y has (n*L)/M samples. */
int skdsp_fir_updn(skdsp_handle h, const void *x, int64_t n, int L, int M, void *y);
int skdsp_fir_updn_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev);

/* ---- FIR bank: sigsys.fft_caf (sigsys.py:2696-2781) ------------------------ */
/* nbands frequency-shifted copies of ONE FIR over ONE input, all from one pass over the input (csrc/fir_bank.hip):
 *   band j:  g_j[n] = taps[n] * exp(2 pi i ((shifts[j] * n) mod period) / period),   n < ntaps
 * (the reference rolls the 2 n_fft2-point spectrum of the taps by shifts[j] bins: period = 2 n_fft2; the phase is reduced in
 * integers before any sine or cosine).  taps: ntaps float64 (taps_complex = 0) or complex128 (1).  dtype: SKDSP_F32 or
 * SKDSP_C64, the SIGNAL's type; every output row is complex64.  SKDSP_ERR_BADARG unless 1 <= ntaps <= 2049, nbands >= 1,
 * period >= 1 and the band tables (nbands x 32 KiB of transfer functions + nbands x ntaps x 16 bytes of float64 taps for the
 * exact path of non-finite samples) stay within 256 MiB.  The handle is freed by skdsp_destroy. */
int skdsp_fir_bank_create(const void *taps, int ntaps, int taps_complex, const int64_t *shifts, int nbands, int period, int dtype,
                          skdsp_handle *out);
/* y[j * row_stride + m] = sum_{k < ntaps} g_j[k] x[m - k],  x[< 0] = 0,  m < n, j < nbands; row_stride >= n in complex64
 * elements; elements [n, row_stride) of a row are not written. */
int skdsp_fir_bank_dev(skdsp_handle h, const void *x_dev, int64_t n, void *y_dev, int64_t row_stride);

/* Is this cascade one that runs the reference's own recursion, sample by sample (csrc/iir_seq.hip)?  scipy.signal.sosfilt
 * (multirate_helper.py:173) evaluates a cascade section after section in float64; for ill-conditioned designs (a 40th-order Chebyshev)
 * that result is itself good to ~1e-6 only, and a scan would add to it.  skdsp_sos_create probes every cascade of more than 8 sections
 * (the reference's recursion with the sections as given and reversed, on a fixed pseudo-random input); *spread receives the relative
 * difference it found (0 where no probe ran), *is_sequential whether the handle therefore runs sequentially (slow: the reference's own
 * speed).  The Python layer logs a WARNING for such handles. */
int skdsp_iir_sequential(skdsp_handle h, int *is_sequential, double *spread);

/* ---- IIR: multirate_IIR (multirate_helper.py:159-192), rate_change (:54-83) - */
/* sos: nsec x 6 float64, sos[:,3]==1 (scipy.signal.sosfilt contract); any number of sections up to 4096, as sosfilt takes them
 * (more than 8 run as consecutive groups of at most 8 on the device; a float32 cascade whose intermediate signals do not survive
 * float32 storage between two groups runs in float64 inside). */
int skdsp_sos_create(const double *sos, int nsec, int dtype, skdsp_handle *out);
/* transfer function (b,a) for signal.lfilter(b,a,.), multirate_helper.py:74,81;
 * a[0]-normalised.  scipy runs (b,a) as one DF2T section of order N; the scan kernel
 * runs the same transfer function factored into biquads (see iir_design.hpp: the order-N
 * companion coordinates are too ill-conditioned for an affine scan).  Order <= 24. */
int skdsp_tf_create(const double *b, int nb, const double *a, int na, int dtype, skdsp_handle *out);
/* host-only: the (b,a) -> sos factorisation tf_create applies; sos_out holds up to 12x6 doubles */
int skdsp_tf2sos(const double *b, int nb, const double *a, int na, double *sos_out, int *nsec_out);
/* .filter: sosfilt(sos,x) (:169-174) / lfilter(b,a,x) */
int skdsp_iir_filter(skdsp_handle h, const void *x, int64_t n, void *y);
int skdsp_iir_filter_dev(skdsp_handle h, const void *x_dev, int64_t n, void *y_dev);
/* Streaming state (NOT reference behaviour: the reference always starts from
 * rest).  zi / zf are host arrays of skdsp_iir_state_len() doubles: for a real signal the DF2T
 * delays in scipy.signal.sosfilt's zi layout (n_sections x 2); for a complex signal the states of
 * the real-part stream followed by those of the imaginary-part stream.  Handles made by
 * skdsp_tf_create use the layout of their internal biquad cascade (opaque: feed a zf back as zi).
 * zi == NULL means rest; zf == NULL means "not wanted" (no stream synchronisation). */
int skdsp_iir_state_len(skdsp_handle h, int *len);
int skdsp_iir_filter_state_dev(skdsp_handle h, const void *x_dev, int64_t n, const double *zi, double *zf, void *y_dev);
/* N-D inputs: scipy filters along the last axis in ONE call (multirate_helper.py:173: sosfilt(sos, x), x of any
 * shape).  nrow rows of n samples, x_stride / y_stride elements apart (>= n), zero initial state per row, one launch
 * (one staged copy each way for the host-pointer form, rows contiguous).  */
int skdsp_iir_filter_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, void *y);
int skdsp_iir_filter_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev);
/* host-only (no GPU): the partial-fraction expansion the parallel-form scan (csrc/iir_par.hip) runs for the transfer
 * function of an (n_sections x 6) sos array, H(z) = c0 + sum_k (r0_k + r1_k z^-1) / (1 + a1_k z^-1 + a2_k z^-2):
 * out = [c0, (a1, a2, r0, r1) x n_sections, branch-cancellation factor, impulse-response error vs the cascade,
 *        worst probe error of the float32 from-rest states on 128-sample chunks, the same on 96-sample chunks] (5 + 4 n_sections doubles:
 *        float32 / complex64 signals through 7 - 8 biquads form those states on the float32 matrix instruction where the error stays below 5e-7);
 * *accepted = 1 when the expansion passed its acceptance test (else the cascade kernels serve the handle). */
int skdsp_sos_par_info(const double *sos, int nsec, double *out, int *accepted);
/* .up: filter(L*upsample(x,L)) (:69-75, :177-183); y has n*L samples */
int skdsp_iir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y);
int skdsp_iir_up_dev(skdsp_handle h, const void *x_dev, int64_t n, int L, void *y_dev);
/* .dn: downsample(filter(x), M) (:77-83, :186-192); y has n/M samples */
int skdsp_iir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y);
int skdsp_iir_dn_dev(skdsp_handle h, const void *x_dev, int64_t n, int M, void *y_dev);
/* The names SURVEY.md 8(b) sketched for the three calls above on handles made by skdsp_sos_create: the same functions
 * (multirate_IIR.filter / .up / .dn, multirate_helper.py:169-192), kept so that a binding written from that table links. */
int skdsp_sos_filter(skdsp_handle h, const void *x, int64_t n, void *y);
int skdsp_sos_up(skdsp_handle h, const void *x, int64_t n, int L, void *y);
int skdsp_sos_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y);

/* ---- rate-change primitives (sigsys.py:3031-3083) -------------------------- */
/* upsample: y[k*L] = x[k], zeros elsewhere (sigsys.py:3050-3053). y has n*L samples. */
int skdsp_upsample(const void *x, int64_t n, int L, int dtype, void *y);
int skdsp_upsample_dev(const void *x_dev, int64_t n, int L, int dtype, double scale, void *y_dev);
/* downsample: y[k] = x[k*M+p], k < n/M, 0 <= p < M (sigsys.py:3078-3083). */
int skdsp_downsample(const void *x, int64_t n, int M, int p, int dtype, void *y);
int skdsp_downsample_dev(const void *x_dev, int64_t n, int M, int p, int dtype, void *y_dev);
/* farrow: arbitrary-ratio Farrow resampler, digitalcom.farrow_resample(x, fs_old, fs_new, i_ord, alpha)
 * (digitalcom.py:53-235), with Ts_old = 1/fs_old, Ts_new = 1/fs_new.  Output j (0 <= j < n_out) is a 4-tap FIR of x around
 * n_old(j) + 1 whose taps are polynomials of order i_ord (1, 2 or 3; alpha shapes i_ord 2) in the fractional delay mu(j).
 * skdsp_farrow_len: n_out = len(np.arange(0, Ts_old*(n-3) + Ts_old, Ts_new)); host-only, needs no device.
 * skdsp_farrow_dev: outputs [n0, n0 + count) of the whole result into y_dev[0 .. count).
 * wide: bit 0 (SKDSP_FARROW_WIDE) float64 / complex128 results from a float32 / complex64 input, bit 1 (SKDSP_FARROW_F64)
 * float64 arithmetic for such an input (float64 / complex128 inputs always run in float64 and ignore both bits). */
#define SKDSP_FARROW_WIDE 1
#define SKDSP_FARROW_F64 2
int skdsp_farrow_len(int64_t n, double Ts_old, double Ts_new, int64_t *n_out);
int skdsp_farrow_dev(const void *x_dev, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int64_t n0,
                     int64_t count, int wide, void *y_dev);
int skdsp_farrow(const void *x, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int wide, void *y);
/* psd: the Welch primitive of sigsys.psd / my_psd / simple_sa (sigsys.py:2497-2585, 2457-2494, 1008-1084):
 *   S[k] = sum_{i < nseg} | sum_{m < ns} window[m] x[i step + m] exp(-2 pi j k m / n_fft) |^2,   k = 0 .. n_fft-1, float64
 * window: HOST array of ns doubles (used in float64 for every dtype, like the twiddles).  SKDSP_ERR_BADARG unless n_fft is a power of
 * two in 64 ... 4096, 1 <= ns <= n_fft, step >= 1, nseg >= 1 and (nseg-1) step + ns <= n.  Samples behind the last segment
 * are not used; the result is bit-identical from call to call. */
int skdsp_psd_dev(const void *x_dev, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg,
                  double *S_dev);
int skdsp_psd(const void *x, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg, double *S);

/* Viterbi decoding of rate 1/2 and 1/3 convolutional codes, bit for bit fec_conv.FECConv.viterbi_decoder (fec_conv.py:252-499): a
 * register-exchange decoder of decision depth `depth` (1 ... 128) over the 2^(K-1) states of npoly = 2 or 3 polynomials given as strings
 * of K = 3 ... 9 binary digits (csrc/viterbi.hip, csrc/viterbi_core.hpp).  A call takes n received values (2 or 3 per symbol) and writes
 * one byte 0 / 1 per symbol from symbol depth - 1 on: skdsp_viterbi_out_len values.
 *   metric 0 (hard):    xtype 0, int8 values 0 / 1; n need not be a multiple of the values per symbol (a short last symbol counts as it is)
 *   metric 1 (soft):    xtype 1, int16 values ALREADY truncated toward zero, |value| <= 4095; levels 0 and 2^quant_level - 1, quant_level 0 ... 12
 *   metric 2 (unquant): xtype 2, float64 values; levels 0.0 and 1.0
 * skdsp_viterbi_decode continues from the state the handle's previous decode calls left (as the reference object does) and leaves its own;
 * skdsp_viterbi_reset returns the handle to rest; a handle that is not at rest refuses to switch between the integer metrics and unquant.
 * skdsp_viterbi_decode_rows decodes nrow independent rows of n values each (contiguous) from rest in one launch, nrow rows of out_len
 * bytes, and neither reads nor writes the handle's state.  The handle is freed by skdsp_destroy. */
int skdsp_viterbi_create(const char *const *polys, int npoly, int depth, skdsp_handle *out);
int skdsp_viterbi_out_len(skdsp_handle h, int64_t nsym_values, int64_t *n_out);
int skdsp_viterbi_reset(skdsp_handle h);
int skdsp_viterbi_decode(skdsp_handle h, const void *x, int64_t n, int xtype, int metric, int quant_level, uint8_t *y);
int skdsp_viterbi_decode_dev(skdsp_handle h, const void *x_dev, int64_t n, int xtype, int metric, int quant_level, uint8_t *y_dev);
int skdsp_viterbi_decode_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y);
int skdsp_viterbi_decode_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level,
                                  uint8_t *y_dev);

/* Single-error-correcting block codes with n = 2^j - 1, k = n - j, j = 3 ... 16, bit for bit fec_block.FECHamming and fec_block.FECCyclic
 * (fec_block.py:61-423), as three tables of j-bit words (csrc/blockcode.hip, csrc/blockcode_core.hpp):
 *   encode:  p = XOR over { i < k : x[i] = 1 } of enc[i];  code word = x[0..k) followed by bits j-1 ... 0 of p
 *   decode:  s = XOR over { i < n : c[i] = 1 } of syn[i];  out[i] = c[i] ^ (s == trap[i]),  i < k
 * One byte 0 / 1 per bit on both sides: encode takes nblocks * k bytes and writes nblocks * n, decode the reverse; nblocks = 0 is a no-op.
 * The _dev pointers may have any byte alignment; nothing outside the two byte ranges is read or written.  One launch per call.  The handle
 * is freed by skdsp_destroy. */
int skdsp_blockcode_create(int n, int k, const uint32_t *enc /*k*/, const uint32_t *syn /*n*/, const uint32_t *trap /*k*/, skdsp_handle *out);
int skdsp_blockcode_encode(skdsp_handle h, const uint8_t *bits, int64_t nblocks, uint8_t *code);
int skdsp_blockcode_encode_dev(skdsp_handle h, const uint8_t *bits_dev, int64_t nblocks, uint8_t *code_dev);
int skdsp_blockcode_decode(skdsp_handle h, const uint8_t *code, int64_t nblocks, uint8_t *bits);
int skdsp_blockcode_decode_dev(skdsp_handle h, const uint8_t *code_dev, int64_t nblocks, uint8_t *bits_dev);

/* The FEC chain around the Viterbi decoder (csrc/convcode.hip, csrc/convcode_core.hpp): fec_conv.FECConv.conv_encoder, puncture and
 * depuncture (fec_conv.py:501-712) over the rows of a frame set, and the count behind digitalcom.bit_errors (digitalcom.py:353-415).
 * Bits are bytes 0 / 1.  The _dev pointers may have any byte alignment (puncture / depuncture: the element's); nothing outside a row's
 * own bytes is read or written; n = 0 and nrow = 0 are valid and launch nothing.
 *   encode_rows:  nrow rows of n bits -> nrow rows of R n code bits [G1 G2 (G3)] per input bit, the polynomials as for skdsp_viterbi_create
 *                 (the same masks, the reference's rate-1/2 rule included).  A state is one byte: the reference's state string of K - 1
 *                 digits (newest first) read as a binary number.  nstates_in = 0 (rest), 1 (one for all rows) or nrow; states_out (nrow
 *                 bytes, may be null) receives each row's final state.  In the _dev form both state arrays are device pointers.
 *   puncture_rows / depuncture_rows:  rows of n elements of elem_bytes = 1, 2, 4 or 8; digit k of a pattern string is bit k of its mask,
 *                 L_pp <= 64 digits, both masks with the same number of ones; the reference's truncation rule per row
 *                 (skdsp_puncture_out_len / skdsp_depuncture_out_len).  erase: HOST pointer to one element, already in the element type.
 *   bit_count_rows:  counts[r] = the number of i < n with tx[r tx_stride + i] != rx[r rx_stride + i] (invert: with ==), int64; strides
 *                 in bytes, start offsets folded into the pointers; exact and identical from run to run. */
int skdsp_convcode_create(const char *const *polys, int npoly, skdsp_handle *out);
int skdsp_convcode_encode_rows(skdsp_handle h, const uint8_t *bits, int64_t n, int64_t nrow, const uint8_t *states_in, int64_t nstates_in, uint8_t *code,
                               uint8_t *states_out);
int skdsp_convcode_encode_rows_dev(skdsp_handle h, const uint8_t *bits_dev, int64_t n, int64_t nrow, const uint8_t *states_in_dev, int64_t nstates_in,
                                   uint8_t *code_dev, uint8_t *states_out_dev);
int skdsp_puncture_out_len(int64_t n, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out);
int skdsp_depuncture_out_len(int64_t n, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out);
int skdsp_puncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y);
int skdsp_puncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y_dev);
int skdsp_depuncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y);
int skdsp_depuncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase,
                              void *y_dev);
int skdsp_bit_count_rows(const uint8_t *tx, int64_t tx_stride, const uint8_t *rx, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts);
int skdsp_bit_count_rows_dev(const uint8_t *tx_dev, int64_t tx_stride, const uint8_t *rx_dev, int64_t rx_stride, int64_t n, int64_t nrow, int invert,
                             int64_t *counts_dev);

/* Gray symbol mapping (csrc/symmap.hip, csrc/symmap_core.hpp): the symbol sequences of digitalcom.qam_gray_encode_bb / mpsk_gray_encode_bb
 * (digitalcom.py:1584-1681, 1742-1826) and digitalcom.qam_gray_decode / mpsk_gray_decode (digitalcom.py:1684-1739, 1829-1883) over the rows of a
 * frame set.  kind: 0 QAM (mod 2, 4, 16, 64, 256), 1 MPSK (mod 2, 4, 8, 16, 32); dtype: SKDSP_C64 or SKDSP_C128, pointers aligned to the element.
 * Bits are bytes 0 / 1 (bit 0 significant), MSB first within a symbol, at any byte alignment.  Symbol k of an input row is element
 * start + k step of that row (rows x_stride elements apart): nothing else of x is read.  bits_stride: bytes from row to row.
 *   gray_map_rows:   n symbols per row from bps n bytes.  tab_re / tab_im: HOST pointers, the constellation as the caller computed it, already
 *                    rounded to float32 for complex64 output -- QAM of 4 points and more: the ntab = sqrt(mod) levels (tab_im unused), otherwise
 *                    the ntab = mod points.  The kernel only looks up.
 *   qam_scale_rows:  r[row] = 1 / (std(row) c), float64, std = sqrt(sum |x - mean|^2 / n): a deterministic merge of partial moments.
 *   qam_demap_rows:  int16(clip(rint((x r[row] + x_m (1 + 1j)) / 2), 0, x_m)) per component, Gray decoded; r: what qam_scale_rows wrote (or any
 *                    scale of the caller's) -- a DEVICE pointer in the _dev form, not checked.
 *   mpsk_demap_rows: mod(rint(angle(x rot) mod / 2 / pi), mod), Gray decoded; (rot_re, rot_im): the caller's exp(-1j pi / 4), read for mod 4 only. */
int skdsp_gray_map_rows(const uint8_t *bits, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab, int dtype, void *y);
int skdsp_gray_map_rows_dev(const uint8_t *bits_dev, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab,
                            int dtype, void *y_dev, int64_t y_stride);
int skdsp_qam_scale_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r);
int skdsp_qam_scale_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r_dev);
int skdsp_qam_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r, uint8_t *bits);
int skdsp_qam_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r_dev,
                             uint8_t *bits_dev, int64_t bits_stride);
int skdsp_mpsk_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                          uint8_t *bits);
int skdsp_mpsk_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                              uint8_t *bits_dev, int64_t bits_stride);

/* The AWGN channel and the bit sources of the device-resident BER loops (csrc/channel.hip, csrc/channel_core.hpp): sigsys.cpx_awgn / cpx_awgn2
 * (sigsys.py:2335-2454), digitalcom.awgn_channel (digitalcom.py:1259-1281), sigsys.pn_gen (sigsys.py:1947-1980) and random data bits, over the
 * rows of a frame set.  Device pointers only.  The draw is counter based (Philox4x32-10, key = seed, counter = (block, row, tag)): element i of
 * row r depends on (seed, first_row + r, first_index + i) alone, so a window of a row can be generated by itself and two runs are identical.
 * One block is one complex normal (float64, radius up to 8.57 sigma); a real stream's element i is component i & 1 of block i >> 1.
 *   awgn_rows:        y[r, i] = g[r] x[r, i] + sigma[r] z.  y_dtype float32 / float64 (real z) or complex64 / complex128 (complex z); x_dtype
 *                     = y_dtype, or the real dtype of the same precision.  Strides in elements, pointers aligned to the element, y == x allowed.
 *                     g_dev / sigma_dev: nrow float64 on the device (awgn_sigma_rows wrote them), or null to use the scalars g / sigma.
 *   awgn_bits_rows:   bytes 0 / 1 -> the hard decision of 2 b - 1 + sigma z (real z) as bytes: 1, 0, 2 for an exact zero, 3 for not-a-number.
 *   awgn_sigma_rows:  var = np.var(row) by the deterministic merge of partial moments behind qam_scale_rows; mode 0 (cpx_awgn): sigma =
 *                     sqrt(ns var p / 2), g = 1 with p = 10^(-es_n0 / 10); mode 1 (cpx_awgn2): sigma = sqrt(var_w / 2), g = sqrt(1 / ns var_w / var p)
 *                     with p = 10^(es_n0 / 10) and var_w linear.  The powers of ten are the caller's.
 *   random_bits_rows: bit i of row r of the tag-1 stream, one byte each: bit k & 31 of word k >> 5 of block i >> 7, k = i & 127.
 *   pn_rows:          y[r, i] = period[(phases[r] + first_index + i) mod q]; period_dev: q <= 65535 bytes, phases_dev: nrow int64 >= 0 or null.
 * Bits have any byte alignment; strides of bits are bytes.  n = 0 and nrow = 0 are valid and launch nothing. */
int skdsp_awgn_rows_dev(const void *x_dev, int64_t x_stride, int x_dtype, void *y_dev, int64_t y_stride, int y_dtype, int64_t n, int64_t nrow, const double *g_dev,
                        const double *sigma_dev, double g, double sigma, uint64_t seed, int64_t first_index, int64_t first_row);
int skdsp_awgn_bits_rows_dev(const uint8_t *x_dev, int64_t x_stride, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, const double *sigma_dev, double sigma,
                             uint64_t seed, int64_t first_index, int64_t first_row);
int skdsp_awgn_sigma_rows_dev(const void *x_dev, int64_t x_stride, int64_t n, int64_t nrow, int dtype, int mode, double ns, double p, double var_w, double *g_dev,
                              double *sigma_dev);
int skdsp_random_bits_rows_dev(uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, uint64_t seed, int64_t first_index, int64_t first_row);
int skdsp_pn_rows_dev(const uint8_t *period_dev, int q, const int64_t *phases_dev, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, int64_t first_index);

/* OFDM modulation and demodulation over the rows of a frame set (csrc/ofdm.hip, csrc/ofdm_core.hpp): digitalcom.ofdm_tx / ofdm_rx /
 * chan_est_equalize (digitalcom.py:1322-1547; mux_pilot_blocks is index arithmetic inside the transmitter).  complex64 or complex128 rows,
 * computed in float64 and rounded once; strides in elements, pointers aligned to the element; not in place.  nc: a power of two in 64 ... 4096,
 * nf even in 2 ... nc - 2 (carrier c in bin c + 1 for c < nf / 2, else bin nc - nf + c), 0 <= ncp <= nc (ignored unless cp), npb the pilot
 * period: 0 none, >= 2 a pilot (all ones) in front of every npb - 1 data symbols.
 *   ofdm_tx_rows:       nsym data symbols of nf carriers per row -> T (nc + ncp) samples, T = nsym (npb = 0) or nsym + nsym / (npb - 1) + 1; where
 *                       npb - 1 divides nsym the last symbol is all zeros, as in the reference.
 *   ofdm_rx_rows:       nsym received symbols per row (stride nc + ncp behind a prefix of ncp samples with cp, else stride nc) -> the nf carriers of
 *                       its data symbols, (nsym - ceil(nsym / npb)) nf elements for npb > 0, else nsym nf.  hht: the known channel on the nf filled
 *                       carriers, complex128 on the HOST, or null.  npb = -1: every symbol divided by hht.  npb > 0: symbols k with k % npb == 0
 *                       are pilots and run H = z[0], H = alpha H + (1 - alpha) z[k]; data symbols are divided by hht if given (the reference), else
 *                       by the estimate of the latest pilot in front of them; h[r] (nf complex128 per row, npb > 0 only) is the row's last estimate.
 *   ofdm_equalize_rows: the same estimator and division on the rows of a caller's z, nsym symbols of nf carriers each (npb >= 2).
 * nsym = 0 and nrow = 0 are valid. */
int skdsp_ofdm_tx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y);
int skdsp_ofdm_tx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y_dev,
                           int64_t y_stride);
int skdsp_ofdm_rx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha, const double *hht, void *z, void *h);
int skdsp_ofdm_rx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                           const double *hht, void *z_dev, int64_t z_stride, void *h_dev);
int skdsp_ofdm_equalize_rows(const void *z, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht, void *out, void *h);
int skdsp_ofdm_equalize_rows_dev(const void *z_dev, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht,
                                 void *out_dev, int64_t out_stride, void *h_dev);

/* Symbol-error tools of the classical BER loops (csrc/symerr.hip, csrc/symerr_core.hpp): digitalcom.xcorr (digitalcom.py:1163-1179), qam_sep
 * (digitalcom.py:495-582), qpsk_bep (:723-790) and bpsk_bep (:793-846).  Streams are float32 / complex64 / float64 / complex128 (a real stream has
 * imaginary part 0), widened at the load; pointers aligned to the element.
 *   lag_corr:        R[i] = sum_{n < K} a[(n + l) mod K] conj(b[n]), l = first_lag + i, K = 2 floor(len / 2), over the lags the reference keeps:
 *                    first_lag = -min(n_lags, K / 2), n_out = min(2 n_lags + 1, K) (skdsp_lag_corr_len).  r: n_out complex128, e: (sum |a|^2, sum |b|^2);
 *                    in the _dev form both are device pointers, 16-byte aligned.  Sums are float64 in a fixed order: integer-valued streams give exact
 *                    integers, two runs the same bits.  quant_levels = M in {2, 4, 8, 16} passes each component of a through qam_sep's quantiser
 *                    2 clip(rint((M - 1)(v + 1) / 2), 0, M - 1) - (M - 1) at the load; 0: none.  lags (host form): n_out int64, may be null.
 *   sym_count_rows:  per row, over n symbols: tx symbol i = tx[r tx_stride + t0 + i], rx symbol i = x[r x_stride + start + (r0 + i) step], rx rotated by
 *                    (1j)^kphase (mode 2: (-1)^kphase).  mode 0 (QAM, levels = M as above): rx quantised, then rotated; counts[4 r] = symbols whose
 *                    two Gaussian integers differ.  mode 1 (QPSK): with tI = int16((re tx + 1) / 2), rI likewise of rx, tQ / rQ of the imaginary parts,
 *                    counts[4 r ...] = sum(tI ^ rI), sum(tQ ^ rQ), sum((tI ^ rI) | (tQ ^ rQ)) -- the reference's integers, also on soft values.
 *                    mode 2 (BPSK): the real parts only, counts[4 r] = sum(tI ^ rI).  counts[4 r + 3] = the symbols left out because a value is not
 *                    finite, tx is not integer-valued (mode 0) or |(v + 1) / 2| >= 32768 (modes 1, 2): a caller treats a non-zero count as an error.
 *                    Strides in elements; exact and identical from run to run.
 * len = 0, n = 0 and nrow = 0 are valid and launch nothing. */
int skdsp_lag_corr_len(int64_t len, int64_t n_lags, int64_t *n_out, int64_t *first_lag);
int skdsp_lag_corr(const void *a, int a_dtype, const void *b, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, int64_t *lags, void *r, double *e);
int skdsp_lag_corr_dev(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, void *r_dev, double *e_dev);
int skdsp_sym_count_rows(const void *tx, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                         int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts);
int skdsp_sym_count_rows_dev(const void *tx_dev, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x_dev, int x_dtype, int64_t x_stride, int64_t start,
                             int64_t step, int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts_dev);

/* Pulse shaping and matched filtering over the rows of a frame set (csrc/pulse.hip, csrc/pulse_core.hpp): the two filtering stages of a single-carrier
 * BER loop, every row a frame that starts from rest.  b: ntaps real float64 taps; dtype: the signal's (any of the four).
 *   pulse_shape_rows:  y[r, k ns + p] = c * sum_j b[p + j ns] x[r, k - j] (0 <= p < ns, 0 <= k < n, every j with p + j ns < ntaps) -- per row
 *                      lfilter(b, 1, upsample(x, ns)), n ns outputs.  scale: null, or a HOST pointer to the real factor c (one float64 multiplication per
 *                      component behind the sum).
 *   pulse_mf_rows:     y[r, k] = sum_i b[i] x[r, start + k step - i], 0 <= k < n_out = max(0, ceil((n - start) / step)) (skdsp_pulse_mf_out_len) -- per
 *                      row lfilter(b, 1, x)[start::step]; step = 1 is a plain from-rest FIR over the rows.
 * One arithmetic recipe for every dtype: elements widened exactly, float64 products and sums without fused multiply-adds, the terms of an output added
 * from the oldest sample to the newest (acc = b x + acc from +0), real and imaginary parts apart, one rounding at the store -- identical from run to run
 * and to the NumPy restatements of the Python layer.  _dev forms: x_stride / y_stride elements between rows as in skdsp_fir_filter_rows_dev; host forms:
 * rows contiguous.  SKDSP_ERR_BADARG unless x_stride >= n and y_stride >= the output row length, and where input and output overlap (in place is not
 * supported); SKDSP_ERR_UNSUPPORTED outside 1 <= ns, step <= 64 and ntaps <= 2049.  n = 0 and nrow = 0 are valid and launch nothing.  The handle is
 * freed by skdsp_destroy. */
int skdsp_pulse_create(const double *b, int ntaps, int dtype, skdsp_handle *out);
int skdsp_pulse_mf_out_len(int64_t n, int64_t start, int64_t step, int64_t *n_out);
int skdsp_pulse_shape_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int ns, const double *scale, void *y);
int skdsp_pulse_shape_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int ns, const double *scale, void *y_dev, int64_t y_stride);
int skdsp_pulse_mf_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int64_t start, int64_t step, void *y);
int skdsp_pulse_mf_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, void *y_dev, int64_t y_stride);

/* Decision-directed carrier phase tracking over the rows of a frame set (csrc/carrier.hip, csrc/carrier_core.hpp): synchronization.DD_carrier_sync per row, every
 * row a frame from rest (theta_hat = 0, vi = 0), and the impairment helpers phase_step / time_step.  dtype: complex64 or complex128 (complex64 is storage only:
 * the loop runs in float64).  Symbol k of a row is element start + k step; n: the symbols of a row; strides in elements; no handle.
 *   carrier_rows:    per symbol z' = z exp(-1j theta_hat), the decision a_hat (family 0 QAM of mod 2, 4, 16, 64, 256; 1 MPSK of mod 2 ... 32), the detector
 *                    (type 0 im(z') re(a) - re(z') im(a), 1 the wrapped angle difference, 2 im(z' / a)), vi += k2 e, theta_hat = mod(theta_hat + k1 e + vi, 2 pi).
 *                    outputs: bit 0 z_prime, 1 a_hat (both of dtype), 2 e_phi, 3 theta_h (float64): only the selected ones are written (the others may be null);
 *                    y_stride serves all four.  gains: null (k1, k2 serve every row) or nrow pairs (k1, k2).  r_dev: QAM, the rows' 1 / (std c) as
 *                    skdsp_qam_scale_rows_dev writes them (the host form makes them itself from qam_c = sqrt(3 / (2 (mod - 1)))).  inv_sqrt2: the caller's
 *                    1 / sqrt(2) (MPSK 4); tab_re, tab_im: HOST pointers to the mod decision points exp(1j 2 pi a / mod) (MPSK above 4), else null.
 *   time_step_rows:  y[r, j] = x[r, j] for j < min(n, ns n_step), else x[r, j + t_step] where that lies inside the row, else 0; j < n_out.  t_steps_dev:
 *                    null or nrow int64 on the device.
 *   phase_step_rows: y[r, j] = x[r, j ns] f, j < ceil(n / ns), f = 1 + 0j before n_step and (f_re, f_im), the caller's exp(1j p_step), from there on;
 *                    factors_dev: null or nrow pairs on the device.
 * The device, the host emulation (tests/host/carrier_emul.cpp) and the NumPy restatement (_ffi.dd_carrier_rows_host) give the same bits. */
int skdsp_carrier_rows(const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop, double k1,
                       double k2, const double *gains, double qam_c, double inv_sqrt2, const double *tab_re, const double *tab_im, int outputs, void *z, void *a, double *e,
                       double *t);
int skdsp_carrier_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop,
                           double k1, double k2, const double *gains_dev, const double *r_dev, double inv_sqrt2, const double *tab_re, const double *tab_im, int outputs,
                           void *z_dev, void *a_dev, double *e_dev, double *t_dev, int64_t y_stride);
int skdsp_time_step_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, int64_t t_step, const int64_t *t_steps_dev,
                             void *y_dev, int64_t n_out, int64_t y_stride);
int skdsp_phase_step_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, double f_re, double f_im,
                              const double *factors_dev, void *y_dev, int64_t y_stride);

/* Non-data-aided symbol timing recovery over the rows of a frame set (csrc/timing.hip, csrc/timing_core.hpp): synchronization.NDA_symb_sync per row, every row a
 * frame from rest.  dtype: complex64 or complex128 (complex64 is storage only: the loop runs in float64).  A row's frame is x[r, start ... start + n - 1]; strides in
 * elements; no handle.  ns: samples per symbol, 2 ... 16; L: the detector is smoothed over 2L + 1 symbols, 0 ... 8; iord: the Farrow interpolator's order, 1, 2 or 3;
 * (k1, k2) or gains (nrow pairs): the loop filter's gains; rot: ns real parts, then ns imaginary parts, of exp(-1j 2 pi k / ns) on the HOST; inv_ns = 1 / ns,
 * inv_len = 1 / (2L + 1), k_eps = -1 / (2 pi) as the caller's arithmetic rounds them.  outputs: bit 0 zz (of dtype), 1 e_tau (float64): only the selected ones are
 * written.  counts[r] is the reference's output length of row r; a row's outputs take min(counts[r], cap) elements and nothing behind them is written by the device
 * form (the host form returns zeros there).  counts[r] > cap tells the caller that the row was cut.  normalize: zz /= np.std(zz) per row.  For ns = 2 with
 * iord >= 2 a frame of odd length >= 3 is refused: the reference's own slices run past its array there.
 * The device, the host emulation (tests/host/nda_emul.cpp) and the NumPy restatement (_ffi.nda_rows_host) give the same bits. */
int skdsp_nda_rows(const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2, const double *gains,
                   const double *rot, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *zz, double *e_tau, int64_t *counts);
int skdsp_nda_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2,
                       const double *gains_dev, const double *rot, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *zz_dev,
                       double *e_tau_dev, int64_t *counts_dev, int64_t y_stride);

/* Host-pointer entry points of a float32/complex64 handle deliver y as float64/complex128 (the
 * reference's result dtype, multirate_helper.py:108 etc.): widened on the device before the copy
 * back, so y must hold twice the bytes.  Device-pointer (_dev) entry points are not affected. */
/* The chunk planner of the host-pointer entry points (long vectors are pipelined in chunks of 2^chunk_log2 samples that
 * are exact continuations of each other): ranges of chunk k.  Host-only, for tests and for callers who stream themselves. */
int skdsp_host_chunk_plan(int64_t n, int L, int M, int64_t hist, int chunk_log2, int64_t k, int64_t *nchunks, int64_t *in_begin,
                          int64_t *in_end, int64_t *in_hist, int64_t *out_begin, int64_t *out_end);
int skdsp_set_wide_output(skdsp_handle h, int on);
int skdsp_destroy(skdsp_handle h);

/* ---- sample-block sharding across GPUs (one process per GPU, RCCL) ------- */
/* rank 0 creates the 128-byte RCCL unique id; the launcher hands it to every rank. */
int skdsp_dist_unique_id(void *id128);
int skdsp_dist_init(int rank, int world, const void *id128);
int skdsp_dist_shutdown(void);
int skdsp_dist_comm_count(int *nranks);           /* ncclCommCount of the live communicator; 0 = none (1-rank job) */
int skdsp_dist_barrier(void);                     /* 1-element RCCL all-reduce + stream sync */
int skdsp_dist_allreduce_max(double *value);      /* in-place max over ranks */
int skdsp_dist_allreduce_sum(double *value);
/* one grouped RCCL point-to-point step on the library stream: send `bytes` to rank dst and
 * receive `bytes` from rank src (either may be -1 = none).  The halo exchange is built on it. */
int skdsp_dist_sendrecv(const void *send_dev, int dst, void *recv_dev, int src, int64_t bytes);
/* every rank contributes `bytes` bytes; recv_dev holds world*bytes, rank-major (IIR end states:
 * sharding.ShardedIIR).  One rank / no communicator: a device copy. */
int skdsp_dist_allgather(const void *send_dev, void *recv_dev, int64_t bytes);
/* Halo exchange for a contiguous sample-block shard: send my LAST n_halo samples of
 * x_dev (n local samples) to rank+1, receive rank-1's into x_dev[-n_halo..-1]
 * (rank 0 zero-fills).  x_dev must have n_halo samples of headroom before it. */
int skdsp_dist_halo_exchange(void *x_dev, int64_t n, int64_t n_halo, int dtype);
/* sharded .filter: halo exchange of ntaps-1 samples, then the local filter. */
int skdsp_fir_filter_shard_dev(skdsp_handle h, void *x_dev, int64_t n_local, void *y_dev);

#ifdef __cplusplus
}
#endif
#endif /* SKDSP_H */
