// capi.hip -- the one-call wrappers of the extern "C" boundary of libskdsp_hip.so (see include/skdsp.h): FIR bank,
// resamplers, Farrow resampler, Welch primitive, Viterbi decoder, block codes, the FEC chain around the decoder, Gray symbol mapping, channel, OFDM,
// symbol-error tools, pulse shaping.  The runtime is runtime.hip, the host-pointer chunk pipeline host_pipe.hip, FIR / IIR dispatch fir_api.hip / iir_api.hip.
//
// An entry point that exists as skdsp_X_dev (device pointers) and skdsp_X (host pointers) has ONE body here, X_call(bool host, ...): the handle lookup,
// the *_check call and the early returns stand once (argument errors need no device), and the host form differs in its row strides (contiguous rows,
// derived by the exported wrapper), its host null-pointer checks and the staging around the launch.  The staging is a StagePlan (stage_plan.hpp has
// its rules): declare the pieces, stage_begin, stage_finish(plan, the launch on plan.in_dev() / plan.dev(i)).  In the device form the plan hands the caller's
// pointers through and stages nothing.  Results are copied back in the order declared: a small side result (final states, last estimates, energies)
// stands before the main output, so its copy is the one that waits for the kernels.
#include "api_internal.hpp"

using namespace skdsp;

// skdsp_X_create: the handle the inner X_create makes, stored through a checked out pointer
template <typename F, typename... A> static int create_into(const char *who, skdsp_handle *out, F make, A... args)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "%s_create: null out", who);
    HandleBase *h = nullptr;
    int rc = make(args..., &h);
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
}

// ---------------------------------------------------------------- resamplers
static int upsample_call(bool host, const void *x, int64_t n, int L, int dtype, double scale, void *y)
{
    API_BEGIN;
    if (host) {
        SK_CHECK(dtype_valid(dtype) && n >= 0 && L >= 1, SKDSP_ERR_BADARG, "upsample: bad arguments");
        if (n == 0) return SKDSP_OK;
    } else
        SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "upsample: bad dtype %d", dtype);
    StagePlan p(host);
    p.input(x, (size_t)n * dtype_size(dtype));
    const int iy = p.add_out(y, (size_t)n * L * dtype_size(dtype));
    int rc = stage_begin(p);
    if (rc) return rc;
    return stage_finish(p, upsample_launch(p.in_dev(), n, L, dtype, scale, p.dev(iy), ctx().stream));
}

static int downsample_call(bool host, const void *x, int64_t n, int M, int phase, int dtype, void *y)
{
    API_BEGIN;
    if (host) {
        SK_CHECK(dtype_valid(dtype) && n >= 0 && M >= 1, SKDSP_ERR_BADARG, "downsample: bad arguments");
        SK_CHECK(phase >= 0 && phase < M, SKDSP_ERR_BADARG, "downsample: phase p=%d out of range for M=%d", phase, M);
        if (n / M == 0) return SKDSP_OK;
    } else
        SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "downsample: bad dtype %d", dtype);
    StagePlan p(host);
    p.input(x, (size_t)n * dtype_size(dtype));
    const int iy = p.add_out(y, host ? (size_t)(n / M) * dtype_size(dtype) : 0);
    int rc = stage_begin(p);
    if (rc) return rc;
    return stage_finish(p, downsample_launch(p.in_dev(), n, M, phase, dtype, p.dev(iy), ctx().stream));
}

// ---------------------------------------------------------------- Farrow resampler
// host form: the whole output, n0 = 0 and count = farrow_len
static int farrow_call(bool host, const void *x, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int64_t n0, int64_t count, int wide, void *y)
{
    API_BEGIN;
    if (host) {
        SK_CHECK(dtype_valid(dtype) && n >= 0, SKDSP_ERR_BADARG, "farrow: bad arguments");
        SK_CHECK(i_ord >= 1 && i_ord <= 3, SKDSP_ERR_BADARG, "farrow: i_ord must be 1, 2 or 3 (got %d)", i_ord);
        int rc = farrow_len(n, Ts_old, Ts_new, &count);
        if (rc || count == 0) return rc;
    }
    const size_t esz_out = dtype_size(dtype) * (!dtype_double(dtype) && (wide & SKDSP_FARROW_WIDE) ? 2 : 1);
    StagePlan p(host);
    p.input(x, (size_t)n * dtype_size(dtype));
    const int iy = p.add_out(y, (size_t)count * esz_out);
    int rc = stage_begin(p);
    if (rc) return rc;
    return stage_finish(p, farrow_launch(p.in_dev(), n, dtype, Ts_old, Ts_new, i_ord, alpha, n0, count, wide, p.dev(iy), ctx().stream));
}

// ---------------------------------------------------------------- Welch primitive (sigsys.psd, my_psd, simple_sa)
static int psd_call(bool host, const void *x, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg, double *S)
{
    int rc = psd_check(n, dtype, window, ns, n_fft, step, nseg);
    if (rc) return rc;
    if (host) {
        SK_CHECK(x && S, SKDSP_ERR_BADARG, "psd: null pointer");
        n = (nseg - 1) * step + ns;   // samples behind the last segment are not even copied
    }
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)n * dtype_size(dtype));
    const int iS = p.add_out(S, (size_t)n_fft * sizeof(double));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, psd_launch(p.in_dev(), n, dtype, window, ns, n_fft, step, nseg, (double *)p.dev(iS), ctx().stream));
}

// ---------------------------------------------------------------- Viterbi decoder (fec_conv.FECConv.viterbi_decoder)
static int viterbi_call(bool host, skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y, int stateful)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_VITERBI);
    SK_CHECK(h, SKDSP_ERR_BADARG, "viterbi: not a Viterbi handle");
    int rc = viterbi_check(h, n, nrow, xtype, metric, quant_level, stateful);
    if (rc) return rc;
    int64_t n_out = 0;
    if (host) {
        SK_CHECK(x, SKDSP_ERR_BADARG, "viterbi: null pointer");
        if ((rc = viterbi_out_len(h, n, &n_out))) return rc;
        SK_CHECK(y || n_out == 0, SKDSP_ERR_BADARG, "viterbi: null pointer");
        if (!stateful && n_out == 0) return SKDSP_OK;
    }
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    StagePlan p(host);
    p.input(x, (size_t)n * (size_t)nrow * (xtype == 0 ? 1 : xtype == 1 ? 2 : 8));
    const int iy = p.add_out(y, (size_t)n_out * (size_t)nrow);   // (nothing comes back from a stateful call that only advances the state)
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, viterbi_launch(h, p.in_dev(), n, nrow, xtype, metric, quant_level, (uint8_t *)p.dev(iy), stateful, ctx().stream));
}

// ---------------------------------------------------------------- block codes (fec_block.FECHamming, fec_block.FECCyclic)
static int blockcode_call(bool host, skdsp_handle hh, int mode, const uint8_t *in, int64_t nblocks, uint8_t *out)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_BLOCKCODE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "blockcode: not a block code handle");
    int rc = blockcode_check(h, nblocks);
    if (rc || nblocks == 0) return rc;
    SK_CHECK(in && out, SKDSP_ERR_BADARG, "blockcode: null pointer");
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    int n = 0, k = 0;
    blockcode_sizes(h, &n, &k);
    StagePlan p(host);
    p.input(in, (size_t)nblocks * (size_t)(mode == 0 ? k : n));
    const int io = p.add_out(out, (size_t)nblocks * (size_t)(mode == 0 ? n : k));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, blockcode_launch(h, mode, (const uint8_t *)p.in_dev(), nblocks, (uint8_t *)p.dev(io), ctx().stream));
}

// ---------------------------------------------------------------- the FEC chain around the decoder (FECConv.conv_encoder / puncture / depuncture, digitalcom.bit_errors)
static int convcode_call(bool host, skdsp_handle hh, const uint8_t *bits, int64_t n, int64_t nrow, const uint8_t *states_in, int64_t nstates_in, uint8_t *code,
                         uint8_t *states_out)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_CONVCODE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "convcode: not a convolutional code handle");
    int rc = convcode_check(h, n, nrow, nstates_in);
    if (rc || nrow == 0) return rc;
    SK_CHECK(nstates_in == 0 || states_in, SKDSP_ERR_BADARG, "convcode: null initial states");
    int K = 0, R = 0;
    convcode_sizes(h, &K, &R);
    if (host) {
        for (int64_t r = 0; r < nstates_in; ++r)
            SK_CHECK(states_in[r] < (1 << (K - 1)), SKDSP_ERR_BADARG, "convcode: state %d of row %lld does not fit the %d state bits", (int)states_in[r], (long long)r, K - 1);
        if (n == 0) {   // nothing to encode: the states pass through
            for (int64_t r = 0; states_out && r < nrow; ++r) states_out[r] = nstates_in == 0 ? 0 : states_in[nstates_in == 1 ? 0 : r];
            return SKDSP_OK;
        }
    }
    SK_CHECK(n == 0 || (bits && code), SKDSP_ERR_BADARG, "convcode: null pointer");
    if (n == 0 && !states_out) return SKDSP_OK;
    API_BEGIN;
    StagePlan p(host);
    p.input(bits, (size_t)n * (size_t)nrow);
    const int is = p.add_in(states_in, (size_t)nstates_in), io = p.add_out(states_out, states_out ? (size_t)nrow : 0);
    const int ic = p.add_out(code, (size_t)n * (size_t)nrow * (size_t)R);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, convcode_launch(h, (const uint8_t *)p.in_dev(), n, nrow, (const uint8_t *)p.dev(is), nstates_in, (uint8_t *)p.dev(ic),
                                           states_out ? (uint8_t *)p.dev(io) : nullptr, ctx().stream));
}

static int gather_call(bool host, int dep, const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y)
{
    int64_t n_out = 0;
    int rc = gather_check(dep, n, nrow, elem_bytes, mask1, mask2, L_pp, &n_out);
    if (rc) return rc;
    SK_CHECK(!dep || erase, SKDSP_ERR_BADARG, "depuncture: null erase value");
    if (nrow == 0 || n_out == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "%s: null pointer", dep ? "depuncture" : "puncture");
    if (!host) SK_CHECK(elem_aligned(x, y, elem_bytes), SKDSP_ERR_BADARG, "%s: the pointers must be aligned to the element", dep ? "depuncture" : "puncture");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)n * (size_t)nrow * (size_t)elem_bytes);
    const int iy = p.add_out(y, (size_t)n_out * (size_t)nrow * (size_t)elem_bytes);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, gather_launch(dep, p.in_dev(), n, nrow, elem_bytes, mask1, mask2, L_pp, erase, p.dev(iy), ctx().stream));
}

// host form: both streams are copied whole -- (nrow - 1) stride + n bytes each
static int bit_count_call(bool host, const uint8_t *tx, int64_t tx_stride, const uint8_t *rx, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts)
{
    int rc = bitcount_check(tx_stride, rx_stride, n, nrow);
    if (rc || nrow == 0) return rc;
    if (host) {
        SK_CHECK(counts, SKDSP_ERR_BADARG, "bit_count: null counts");
        if (n == 0) {
            for (int64_t r = 0; r < nrow; ++r) counts[r] = 0;
            return SKDSP_OK;
        }
    } else
        SK_CHECK(counts && ((uintptr_t)counts & 7) == 0, SKDSP_ERR_BADARG, "bit_count: the counts must be an 8-byte aligned pointer");
    SK_CHECK(n == 0 || (tx && rx), SKDSP_ERR_BADARG, "bit_count: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(tx, (size_t)((nrow - 1) * tx_stride + n));
    const int ir = p.add_in(rx, (size_t)((nrow - 1) * rx_stride + n)), ic = p.add_out(counts, (size_t)nrow * sizeof(int64_t));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, bitcount_launch((const uint8_t *)p.in_dev(), tx_stride, (const uint8_t *)p.dev(ir), rx_stride, n, nrow, invert, (int64_t *)p.dev(ic), ctx().stream));
}

// ---------------------------------------------------------------- Gray symbol mapping (symmap.hip): qam_gray_encode_bb / mpsk_gray_encode_bb's symbols, qam_gray_decode / mpsk_gray_decode
// host form: contiguous rows -- nrow x (bps n) bytes in, nrow x n points out
static int gray_map_call(bool host, const uint8_t *bits, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab,
                         int dtype, void *y, int64_t y_stride)
{
    int rc = symmap_check(kind, mod, n, nrow, dtype, bits_stride, y_stride);
    if (rc) return rc;
    SK_CHECK(tab_re, SKDSP_ERR_BADARG, "gray_map: null table");
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(bits && y, SKDSP_ERR_BADARG, "gray_map: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(bits, (size_t)bits_stride * (size_t)nrow);
    const int iy = p.add_out(y, (size_t)y_stride * (size_t)nrow * dtype_size(dtype));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, symmap_launch((const uint8_t *)p.in_dev(), bits_stride, n, nrow, kind, mod, tab_re, tab_im, ntab, dtype, p.dev(iy), y_stride, ctx().stream));
}

// host forms of the strided calls: the rows are copied whole -- (nrow - 1) x_stride + start + (n - 1) step + 1 elements
static size_t sym_span(int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow) { return (size_t)((nrow - 1) * x_stride + start + (n - 1) * step + 1); }

// the partial moments of a launch live in workspace 3 of the calling slot
static int qam_scale_call(bool host, const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r)
{
    int rc = symscale_check(mod, n, nrow, dtype, x_stride, start, step);
    if (rc || nrow == 0) return rc;
    SK_CHECK(n >= 1, SKDSP_ERR_BADARG, "qam_scale: a row has no symbols");
    SK_CHECK(x && r, SKDSP_ERR_BADARG, "qam_scale: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, sym_span(x_stride, start, step, n, nrow) * dtype_size(dtype));
    const int ir = p.add_out(r, (size_t)nrow * sizeof(double));
    p.scratch_bytes = symscale_scratch_bytes(n, nrow) + 256;
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, symscale_launch(p.in_dev(), x_stride, start, step, n, nrow, dtype, mod, c, p.scratch, (double *)p.dev(ir), ctx().stream));
}

// both demappers: r: the rows' scales (QAM only; host form: a HOST pointer); host form: bits are nrow contiguous rows of bps n bytes
static int demap_call(bool host, int kind, const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r,
                      double rot_re, double rot_im, uint8_t *bits, int64_t bits_stride)
{
    int rc = symdemap_check(kind, mod, n, nrow, dtype, x_stride, start, step, bits_stride);
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x && bits && (kind || r), SKDSP_ERR_BADARG, "%s: null pointer", kind ? "mpsk_demap" : "qam_demap");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, sym_span(x_stride, start, step, n, nrow) * dtype_size(dtype));
    const int ib = p.add_out(bits, (size_t)bits_stride * (size_t)nrow), ir = p.add_in(r, kind ? 0 : (size_t)nrow * sizeof(double));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, symdemap_launch(p.in_dev(), x_stride, start, step, n, nrow, dtype, kind, mod, kind ? nullptr : (const double *)p.dev(ir), rot_re, rot_im,
                                           (uint8_t *)p.dev(ib), bits_stride, ctx().stream));
}

// ---------------------------------------------------------------- OFDM (ofdm.hip): ofdm_tx / ofdm_rx / chan_est_equalize over rows
// host forms: contiguous rows, so the strides are the row lengths.  The pilots, the estimates, the raw data rows and the channel table of a launch
// live in workspace 3 of the calling slot
static int ofdm_tx_call(bool host, const void *x, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y,
                        int64_t y_stride)
{
    int rc = ofdm_tx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, x_stride, y_stride);
    if (rc || nrow == 0) return rc;
    if (host) {
        if (y_stride == 0) return SKDSP_OK;
        SK_CHECK(y && (x || x_stride == 0), SKDSP_ERR_BADARG, "ofdm_tx: null pointer");
    }
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)x_stride * (size_t)nrow * dtype_size(dtype));
    const int iy = p.add_out(y, (size_t)y_stride * (size_t)nrow * dtype_size(dtype));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, ofdm_tx_launch(p.in_dev(), x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, p.dev(iy), y_stride, ctx().stream));
}

static int ofdm_rx_call(bool host, const void *x, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                        const double *hht, void *z, int64_t z_stride, void *h)
{
    int rc = ofdm_rx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, hht != nullptr, x_stride, z_stride);
    if (rc || nrow == 0 || nsym == 0) return rc;
    if (host) SK_CHECK(x && (z || z_stride == 0) && (h || npb <= 0), SKDSP_ERR_BADARG, "ofdm_rx: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)x_stride * (size_t)nrow * dtype_size(dtype));
    const int ih = p.add_out(h, npb > 0 ? (size_t)nrow * nf * 16 : 0), iz = p.add_out(z, (size_t)z_stride * (size_t)nrow * dtype_size(dtype));
    p.scratch_bytes = ofdm_scratch_bytes(nsym, nrow, nf);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, ofdm_rx_launch(p.in_dev(), x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, alpha, hht, p.scratch, p.dev(iz), z_stride, p.dev(ih), ctx().stream));
}

static int ofdm_equalize_call(bool host, const void *z, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht, void *out,
                              int64_t out_stride, void *h)
{
    int rc = ofdm_equalize_check(nsym, nrow, dtype, nf, npb, z_stride, out_stride);
    if (rc || nrow == 0 || nsym == 0) return rc;
    if (host) SK_CHECK(z && h && (out || out_stride == 0), SKDSP_ERR_BADARG, "ofdm_equalize: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(z, (size_t)z_stride * (size_t)nrow * dtype_size(dtype));
    const int ih = p.add_out(h, (size_t)nrow * nf * 16), io = p.add_out(out, (size_t)out_stride * (size_t)nrow * dtype_size(dtype));
    p.scratch_bytes = ofdm_scratch_bytes(nsym, nrow, nf);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, ofdm_equalize_launch(p.in_dev(), z_stride, nsym, nrow, dtype, nf, npb, alpha, hht, p.scratch, p.dev(io), out_stride, p.dev(ih), ctx().stream));
}

// ---------------------------------------------------------------- symbol-error tools (symerr.hip): xcorr / qam_sep / qpsk_bep / bpsk_bep
// host form: the first K elements of both streams are copied, and lags (where given) is filled on the host.  The partials of a launch live in
// workspace 3 of the calling slot
static int lag_corr_call(bool host, const void *a, int a_dtype, const void *b, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, int64_t *lags, void *r, double *e)
{
    int64_t nl = 0, l0 = 0;
    int rc = lagcorr_check(len, n_lags, a_dtype, b_dtype, quant_levels, &nl, &l0);
    if (rc) return rc;
    if (lags)
        for (int64_t i = 0; i < nl; ++i) lags[i] = l0 + i;
    if (nl == 0) return SKDSP_OK;
    SK_CHECK(a && b && r && e, SKDSP_ERR_BADARG, "lag_corr: null pointer");
    API_BEGIN;
    const int64_t K = 2 * (len / 2);
    StagePlan p(host);
    p.input(a, (size_t)K * dtype_size(a_dtype));
    const int ib = p.add_in(b, (size_t)K * dtype_size(b_dtype)), ie = p.add_out(e, 2 * sizeof(double)), ir = p.add_out(r, (size_t)nl * 16);
    p.scratch_bytes = lagcorr_scratch_bytes(len, n_lags);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, lagcorr_launch(p.in_dev(), a_dtype, p.dev(ib), b_dtype, len, n_lags, quant_levels, p.scratch, p.dev(ir), (double *)p.dev(ie), ctx().stream));
}

// host form: both arrays are copied whole -- through the last element a row reads
static int sym_count_call(bool host, const void *tx, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                          int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts)
{
    int rc = symcount_check(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase);
    if (rc || nrow == 0) return rc;
    if (host) {
        SK_CHECK(counts, SKDSP_ERR_BADARG, "sym_count: null counts");
        if (n == 0) {
            for (int64_t i = 0; i < 4 * nrow; ++i) counts[i] = 0;
            return SKDSP_OK;
        }
    } else
        SK_CHECK(counts && ((uintptr_t)counts & 7) == 0, SKDSP_ERR_BADARG, "sym_count: the counts must be an 8-byte aligned pointer");
    SK_CHECK(n == 0 || (tx && x), SKDSP_ERR_BADARG, "sym_count: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(tx, (size_t)((nrow - 1) * tx_stride + t0 + n) * dtype_size(tx_dtype));
    const int ix = p.add_in(x, (size_t)((nrow - 1) * x_stride + start + (r0 + n - 1) * step + 1) * dtype_size(x_dtype));
    const int ic = p.add_out(counts, (size_t)nrow * 4 * sizeof(int64_t));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, symcount_launch(p.in_dev(), tx_dtype, tx_stride, t0, p.dev(ix), x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, (int64_t *)p.dev(ic), ctx().stream));
}

// ---------------------------------------------------------------- pulse shaping and matched filtering over rows (pulse.hip): sigsys.pulse_shape_rows / matched_filter_rows
// host form: rows contiguous in x (n each) and in y (n ns each)
static int pulse_shape_call(bool host, skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int64_t x_stride, int ns, const double *scale, void *y, int64_t y_stride)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_shape: not a pulse handle");
    int rc = pulse_shape_check(h, n, nrow, ns, x_stride, y_stride);
    if (rc || n == 0 || nrow == 0) return rc;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "pulse_shape: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)x_stride * (size_t)nrow * dtype_size(h->dtype));
    const int iy = p.add_out(y, (size_t)y_stride * (size_t)nrow * dtype_size(h->dtype));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, pulse_shape_launch(h, p.in_dev(), n, nrow, ns, x_stride, y_stride, scale != nullptr, scale ? *scale : 1.0, p.dev(iy), ctx().stream));
}

// host form: rows contiguous in x (n each) and in y (skdsp_pulse_mf_out_len each, which the body derives: y_stride is not read)
static int pulse_mf_call(bool host, skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, void *y, int64_t y_stride)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_mf: not a pulse handle");
    int rc = SKDSP_OK;
    if (host && step >= 1 && step <= 64) rc = pulse_mf_out_len(n, start, step, &y_stride);   // (a step the kernel does not take: the check below says so)
    if (rc) return rc;
    rc = pulse_mf_check(h, n, nrow, start, step, x_stride, y_stride);
    if (rc || nrow == 0 || n <= start) return rc;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "pulse_mf: null pointer");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, (size_t)x_stride * (size_t)nrow * dtype_size(h->dtype));
    const int iy = p.add_out(y, (size_t)y_stride * (size_t)nrow * dtype_size(h->dtype));
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, pulse_mf_launch(h, p.in_dev(), n, nrow, start, step, x_stride, y_stride, p.dev(iy), ctx().stream));
}

// ---------------------------------------------------------------- carrier phase tracking and its impairment helpers over rows (carrier.hip): synchronization.DD_carrier_sync_rows,
// phase_step_rows, time_step_rows
// host form: rows x_stride apart in x, contiguous (n each) in the selected outputs; gains: null or nrow pairs on the HOST; the MQAM scales are made here, by the merge
// behind skdsp_qam_scale_rows, in workspace 3 of the calling slot (the device form is handed them)
static int carrier_call(bool host, const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type,
                        int open_loop, double k1, double k2, const double *gains, const double *r, double qam_c, double inv_sqrt2, const double *tab_re, const double *tab_im,
                        int outputs, void *z, void *a, double *e, double *t, int64_t y_stride)
{
    int rc = carrier_check(family, mod, type, dtype, outputs, n, nrow, start, step, x_stride, y_stride);
    if (rc || n == 0 || nrow == 0) return rc;
    SK_CHECK(x, SKDSP_ERR_BADARG, "carrier_rows: null pointer");
    SK_CHECK((!(outputs & 1) || z) && (!(outputs & 2) || a) && (!(outputs & 4) || e) && (!(outputs & 8) || t), SKDSP_ERR_BADARG, "carrier_rows: a selected output is null");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, sym_span(x_stride, start, step, n, nrow) * dtype_size(dtype));
    const size_t rows = (size_t)y_stride * (size_t)nrow;
    const int ig = p.add_in(gains, gains ? (size_t)nrow * 2 * sizeof(double) : 0);
    const int iz = p.add_out((outputs & 1) ? z : nullptr, (outputs & 1) ? rows * dtype_size(dtype) : 0), ia = p.add_out((outputs & 2) ? a : nullptr, (outputs & 2) ? rows * dtype_size(dtype) : 0);
    const int ie = p.add_out((outputs & 4) ? e : nullptr, (outputs & 4) ? rows * sizeof(double) : 0), it = p.add_out((outputs & 8) ? t : nullptr, (outputs & 8) ? rows * sizeof(double) : 0);
    const bool scale_here = host && family == 0;
    const size_t part = stage_round(symscale_scratch_bytes(n, nrow));
    if (scale_here) p.scratch_bytes = part + stage_round((size_t)nrow * sizeof(double)) + 256;
    if ((rc = stage_begin(p))) return rc;
    const double *r_dev = r;
    if (scale_here) {
        double *made = reinterpret_cast<double *>(static_cast<char *>(p.scratch) + part);
        if ((rc = symscale_launch(p.in_dev(), x_stride, start, step, n, nrow, dtype, mod, qam_c, p.scratch, made, ctx().stream))) return stage_finish(p, rc);
        r_dev = made;
    }
    return stage_finish(p, carrier_launch(p.in_dev(), n, nrow, x_stride, start, step, dtype, family, mod, type, open_loop, k1, k2, gains ? (const double *)p.dev(ig) : nullptr,
                                          r_dev, inv_sqrt2, tab_re, tab_im, outputs, p.dev(iz), p.dev(ia), (double *)p.dev(ie), (double *)p.dev(it), y_stride, ctx().stream));
}

// only the device forms are exported (the Python layer stages phase_step_rows / time_step_rows itself); the body is the shared shape, so host = true
// would be the host form: contiguous rows (n in, n_out out), per-row values null or nrow of them on the HOST
static int impair_call(bool host, int mode, const void *x, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, int64_t shift,
                       const int64_t *shifts, double c, double d, const double *factors, void *y, int64_t n_out, int64_t y_stride)
{
    int rc = impair_check(mode, dtype, n, n_out, nrow, ns, n_step, x_stride, y_stride);
    if (rc || n_out == 0 || nrow == 0) return rc;
    SK_CHECK(y && (x || n == 0), SKDSP_ERR_BADARG, "%s: null pointer", mode ? "phase_step" : "time_step");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, n ? (size_t)((nrow - 1) * x_stride + n) * dtype_size(dtype) : 0);
    const int iy = p.add_out(y, (size_t)((nrow - 1) * y_stride + n_out) * dtype_size(dtype));
    const int is = p.add_in(shifts, shifts ? (size_t)nrow * sizeof(int64_t) : 0), iff = p.add_in(factors, factors ? (size_t)nrow * 2 * sizeof(double) : 0);
    if ((rc = stage_begin(p))) return rc;
    return stage_finish(p, impair_launch(mode, p.in_dev(), n, nrow, x_stride, dtype, ns, n_step, shift, shifts ? (const int64_t *)p.dev(is) : nullptr, c, d,
                                         factors ? (const double *)p.dev(iff) : nullptr, p.dev(iy), n_out, y_stride, ctx().stream));
}

// ---------------------------------------------------------------- symbol timing recovery over rows (timing.hip): synchronization.NDA_symb_sync_rows
// host form: rows x_stride apart in x, contiguous (cap each) in the selected outputs, which come back zero behind a row's count; gains: null or nrow pairs on the HOST;
// counts: nrow int64 on the host.  The float64 symbols that complex64 rows are normalised from live in workspace 3 of the calling slot, in both forms.
static int nda_call(bool host, const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2,
                    const double *gains, const double *rot, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *z, double *e,
                    int64_t *counts, int64_t y_stride)
{
    int rc = nda_check(ns, L, iord, dtype, outputs, n, nrow, start, x_stride, y_stride, cap);
    if (rc || nrow == 0) return rc;
    SK_CHECK((x || n == 0) && counts && rot, SKDSP_ERR_BADARG, "nda_rows: null pointer");
    SK_CHECK(cap == 0 || ((!(outputs & 1) || z) && (!(outputs & 2) || e)), SKDSP_ERR_BADARG, "nda_rows: a selected output is null");
    API_BEGIN;
    StagePlan p(host);
    p.input(x, n ? (size_t)((nrow - 1) * x_stride + start + n) * dtype_size(dtype) : 0);
    const size_t rows = (size_t)y_stride * (size_t)nrow, zb = (outputs & 1) ? rows * dtype_size(dtype) : 0, eb = (outputs & 2) ? rows * sizeof(double) : 0;
    const int ig = p.add_in(gains, gains ? (size_t)nrow * 2 * sizeof(double) : 0);
    const int iz = p.add_out((outputs & 1) ? z : nullptr, zb), ie = p.add_out((outputs & 2) ? e : nullptr, eb), ic = p.add_out(counts, (size_t)nrow * sizeof(int64_t));
    p.scratch_bytes = nda_scratch_bytes(dtype, outputs, normalize, nrow, cap);
    if ((rc = stage_begin(p))) return rc;
    if (host) {
        if (zb) SK_HIP(hipMemsetAsync(p.dev(iz), 0, zb, ctx().stream));
        if (eb) SK_HIP(hipMemsetAsync(p.dev(ie), 0, eb, ctx().stream));
    }
    return stage_finish(p, nda_launch(p.in_dev(), n, nrow, x_stride, start, dtype, ns, L, iord, k1, k2, gains ? (const double *)p.dev(ig) : nullptr, rot, inv_ns, inv_len, k_eps,
                                      outputs, normalize, cap, p.scratch, p.dev(iz), (double *)p.dev(ie), (int64_t *)p.dev(ic), y_stride, ctx().stream));
}

extern "C" {

// FIR bank (fir_bank.hip): argument errors need no device
int skdsp_fir_bank_create(const void *taps, int ntaps, int taps_complex, const int64_t *shifts, int nbands, int period, int dtype,
                          skdsp_handle *out)
{
    return create_into("fir_bank", out, fir_bank_create, taps, ntaps, taps_complex, shifts, nbands, period, dtype);
}

int skdsp_fir_bank_dev(skdsp_handle hh, const void *x_dev, int64_t n, void *y_dev, int64_t row_stride)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_FIRBANK);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_bank: not a FIR bank handle");
    SK_CHECK(n >= 0 && row_stride >= n, SKDSP_ERR_BADARG, "fir_bank: need 0 <= n <= row_stride (got n = %lld, row_stride = %lld)", (long long)n, (long long)row_stride);
    if (n == 0) return SKDSP_OK;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "fir_bank: null pointer");
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_bank_launch(h, x_dev, n, y_dev, row_stride, ctx().stream);
}

// ---------------------------------------------------------------- resamplers
int skdsp_upsample_dev(const void *x_dev, int64_t n, int L, int dtype, double scale, void *y_dev) { return upsample_call(false, x_dev, n, L, dtype, scale, y_dev); }
int skdsp_upsample(const void *x, int64_t n, int L, int dtype, void *y) { return upsample_call(true, x, n, L, dtype, 1.0, y); }
int skdsp_downsample_dev(const void *x_dev, int64_t n, int M, int p, int dtype, void *y_dev) { return downsample_call(false, x_dev, n, M, p, dtype, y_dev); }
int skdsp_downsample(const void *x, int64_t n, int M, int p, int dtype, void *y) { return downsample_call(true, x, n, M, p, dtype, y); }

// ---------------------------------------------------------------- Farrow resampler
int skdsp_farrow_len(int64_t n, double Ts_old, double Ts_new, int64_t *n_out) { return farrow_len(n, Ts_old, Ts_new, n_out); }

int skdsp_farrow_dev(const void *x_dev, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int64_t n0,
                     int64_t count, int wide, void *y_dev)
{
    return farrow_call(false, x_dev, n, dtype, Ts_old, Ts_new, i_ord, alpha, n0, count, wide, y_dev);
}
int skdsp_farrow(const void *x, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int wide, void *y)
{
    return farrow_call(true, x, n, dtype, Ts_old, Ts_new, i_ord, alpha, 0, 0, wide, y);
}

// ---------------------------------------------------------------- Welch primitive
int skdsp_psd_dev(const void *x_dev, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg,
                  double *S_dev)
{
    return psd_call(false, x_dev, n, dtype, window, ns, n_fft, step, nseg, S_dev);
}
int skdsp_psd(const void *x, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg, double *S)
{
    return psd_call(true, x, n, dtype, window, ns, n_fft, step, nseg, S);
}

// ---------------------------------------------------------------- Viterbi decoder
int skdsp_viterbi_create(const char *const *polys, int npoly, int depth, skdsp_handle *out) { return create_into("viterbi", out, viterbi_create, polys, npoly, depth); }

int skdsp_viterbi_out_len(skdsp_handle hh, int64_t nsym_values, int64_t *n_out)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_VITERBI);
    SK_CHECK(h, SKDSP_ERR_BADARG, "viterbi_out_len: not a Viterbi handle");
    return viterbi_out_len(h, nsym_values, n_out);
}

int skdsp_viterbi_reset(skdsp_handle hh)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_VITERBI);
    SK_CHECK(h, SKDSP_ERR_BADARG, "viterbi_reset: not a Viterbi handle");
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    return viterbi_reset(h, ctx().stream);
}

int skdsp_viterbi_decode(skdsp_handle h, const void *x, int64_t n, int xtype, int metric, int quant_level, uint8_t *y)
{
    return viterbi_call(true, h, x, n, 1, xtype, metric, quant_level, y, 1);
}
int skdsp_viterbi_decode_dev(skdsp_handle h, const void *x_dev, int64_t n, int xtype, int metric, int quant_level, uint8_t *y_dev)
{
    return viterbi_call(false, h, x_dev, n, 1, xtype, metric, quant_level, y_dev, 1);
}
int skdsp_viterbi_decode_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y)
{
    return viterbi_call(true, h, x, n, nrow, xtype, metric, quant_level, y, 0);
}
int skdsp_viterbi_decode_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y_dev)
{
    return viterbi_call(false, h, x_dev, n, nrow, xtype, metric, quant_level, y_dev, 0);
}

// ---------------------------------------------------------------- block codes
int skdsp_blockcode_create(int n, int k, const uint32_t *enc, const uint32_t *syn, const uint32_t *trap, skdsp_handle *out)
{
    return create_into("blockcode", out, blockcode_create, n, k, enc, syn, trap);
}
int skdsp_blockcode_encode(skdsp_handle h, const uint8_t *bits, int64_t nblocks, uint8_t *code) { return blockcode_call(true, h, 0, bits, nblocks, code); }
int skdsp_blockcode_encode_dev(skdsp_handle h, const uint8_t *bits_dev, int64_t nblocks, uint8_t *code_dev) { return blockcode_call(false, h, 0, bits_dev, nblocks, code_dev); }
int skdsp_blockcode_decode(skdsp_handle h, const uint8_t *code, int64_t nblocks, uint8_t *bits) { return blockcode_call(true, h, 1, code, nblocks, bits); }
int skdsp_blockcode_decode_dev(skdsp_handle h, const uint8_t *code_dev, int64_t nblocks, uint8_t *bits_dev) { return blockcode_call(false, h, 1, code_dev, nblocks, bits_dev); }

// ---------------------------------------------------------------- the FEC chain around the decoder
int skdsp_convcode_create(const char *const *polys, int npoly, skdsp_handle *out) { return create_into("convcode", out, convcode_create, polys, npoly); }

int skdsp_convcode_encode_rows_dev(skdsp_handle h, const uint8_t *bits_dev, int64_t n, int64_t nrow, const uint8_t *states_in_dev, int64_t nstates_in,
                                   uint8_t *code_dev, uint8_t *states_out_dev)
{
    return convcode_call(false, h, bits_dev, n, nrow, states_in_dev, nstates_in, code_dev, states_out_dev);
}
int skdsp_convcode_encode_rows(skdsp_handle h, const uint8_t *bits, int64_t n, int64_t nrow, const uint8_t *states_in, int64_t nstates_in, uint8_t *code,
                               uint8_t *states_out)
{
    return convcode_call(true, h, bits, n, nrow, states_in, nstates_in, code, states_out);
}

int skdsp_puncture_out_len(int64_t n, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out)
{
    SK_CHECK(n_out, SKDSP_ERR_BADARG, "puncture_out_len: null n_out");
    return gather_check(0, n, 0, 1, mask1, mask2, L_pp, n_out);
}

int skdsp_depuncture_out_len(int64_t n, uint64_t mask1, uint64_t mask2, int L_pp, int64_t *n_out)
{
    SK_CHECK(n_out, SKDSP_ERR_BADARG, "depuncture_out_len: null n_out");
    return gather_check(1, n, 0, 1, mask1, mask2, L_pp, n_out);
}

int skdsp_puncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y)
{
    return gather_call(true, 0, x, n, nrow, elem_bytes, mask1, mask2, L_pp, nullptr, y);
}
int skdsp_puncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y_dev)
{
    return gather_call(false, 0, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, nullptr, y_dev);
}
int skdsp_depuncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y)
{
    return gather_call(true, 1, x, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y);
}
int skdsp_depuncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y_dev)
{
    return gather_call(false, 1, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y_dev);
}

int skdsp_bit_count_rows_dev(const uint8_t *tx_dev, int64_t tx_stride, const uint8_t *rx_dev, int64_t rx_stride, int64_t n, int64_t nrow, int invert,
                             int64_t *counts_dev)
{
    return bit_count_call(false, tx_dev, tx_stride, rx_dev, rx_stride, n, nrow, invert, counts_dev);
}
int skdsp_bit_count_rows(const uint8_t *tx, int64_t tx_stride, const uint8_t *rx, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts)
{
    return bit_count_call(true, tx, tx_stride, rx, rx_stride, n, nrow, invert, counts);
}

// ---------------------------------------------------------------- Gray symbol mapping
int skdsp_gray_map_rows_dev(const uint8_t *bits_dev, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab,
                            int dtype, void *y_dev, int64_t y_stride)
{
    return gray_map_call(false, bits_dev, bits_stride, n, nrow, kind, mod, tab_re, tab_im, ntab, dtype, y_dev, y_stride);
}
int skdsp_gray_map_rows(const uint8_t *bits, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab, int dtype, void *y)
{
    return gray_map_call(true, bits, sym_bits_per_symbol(kind, mod) * n, n, nrow, kind, mod, tab_re, tab_im, ntab, dtype, y, n);
}

int skdsp_qam_scale_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r_dev)
{
    return qam_scale_call(false, x_dev, x_stride, start, step, n, nrow, dtype, mod, c, r_dev);
}
int skdsp_qam_scale_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r)
{
    return qam_scale_call(true, x, x_stride, start, step, n, nrow, dtype, mod, c, r);
}

int skdsp_qam_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r_dev,
                             uint8_t *bits_dev, int64_t bits_stride)
{
    return demap_call(false, 0, x_dev, x_stride, start, step, n, nrow, dtype, mod, r_dev, 1.0, 0.0, bits_dev, bits_stride);
}
int skdsp_mpsk_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                              uint8_t *bits_dev, int64_t bits_stride)
{
    return demap_call(false, 1, x_dev, x_stride, start, step, n, nrow, dtype, mod, nullptr, rot_re, rot_im, bits_dev, bits_stride);
}
int skdsp_qam_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r, uint8_t *bits)
{
    return demap_call(true, 0, x, x_stride, start, step, n, nrow, dtype, mod, r, 1.0, 0.0, bits, sym_bits_per_symbol(0, mod) * n);
}
int skdsp_mpsk_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                          uint8_t *bits)
{
    return demap_call(true, 1, x, x_stride, start, step, n, nrow, dtype, mod, nullptr, rot_re, rot_im, bits, sym_bits_per_symbol(1, mod) * n);
}

// ---------------------------------------------------------------- the AWGN channel and the bit sources (channel.hip): cpx_awgn / cpx_awgn2 / awgn_channel, random bits, pn_gen
int skdsp_awgn_rows_dev(const void *x_dev, int64_t x_stride, int x_dtype, void *y_dev, int64_t y_stride, int y_dtype, int64_t n, int64_t nrow, const double *g_dev,
                        const double *sigma_dev, double g, double sigma, uint64_t seed, int64_t first_index, int64_t first_row)
{
    int rc = awgn_check(x_dtype, y_dtype, n, nrow, x_stride, y_stride, first_index, first_row);   // (argument errors need no device)
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "awgn: null pointer");
    API_BEGIN;
    return awgn_launch(x_dev, x_stride, x_dtype, y_dev, y_stride, y_dtype, n, nrow, g_dev, sigma_dev, g, sigma, seed, first_index, first_row, ctx().stream);
}

int skdsp_awgn_bits_rows_dev(const uint8_t *x_dev, int64_t x_stride, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, const double *sigma_dev, double sigma,
                             uint64_t seed, int64_t first_index, int64_t first_row)
{
    int rc = chanbits_check("awgn_bits", n, nrow, x_stride, y_stride, first_index, first_row);
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "awgn_bits: null pointer");
    API_BEGIN;
    return chanbits_launch(x_dev, x_stride, y_dev, y_stride, n, nrow, sigma_dev, sigma, seed, first_index, first_row, 0, ctx().stream);
}

int skdsp_random_bits_rows_dev(uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, uint64_t seed, int64_t first_index, int64_t first_row)
{
    int rc = chanbits_check("random_bits", n, nrow, 0, y_stride, first_index, first_row);
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(y_dev, SKDSP_ERR_BADARG, "random_bits: null pointer");
    API_BEGIN;
    return chanbits_launch(nullptr, 0, y_dev, y_stride, n, nrow, nullptr, 0.0, seed, first_index, first_row, 1, ctx().stream);
}

int skdsp_pn_rows_dev(const uint8_t *period_dev, int q, const int64_t *phases_dev, uint8_t *y_dev, int64_t y_stride, int64_t n, int64_t nrow, int64_t first_index)
{
    int rc = pn_check(q, n, nrow, y_stride, first_index);
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(period_dev && y_dev, SKDSP_ERR_BADARG, "pn: null pointer");
    API_BEGIN;
    return pn_launch(period_dev, q, phases_dev, y_dev, y_stride, n, nrow, first_index, ctx().stream);
}

// the partial moments of a launch live in workspace 3 of the calling slot, as for skdsp_qam_scale_rows_dev
int skdsp_awgn_sigma_rows_dev(const void *x_dev, int64_t x_stride, int64_t n, int64_t nrow, int dtype, int mode, double ns, double p, double var_w, double *g_dev,
                              double *sigma_dev)
{
    SK_CHECK(mode == 0 || mode == 1, SKDSP_ERR_BADARG, "awgn_sigma: mode 0 (cpx_awgn) or 1 (cpx_awgn2)");
    SK_CHECK(dtype >= SKDSP_F32 && dtype <= SKDSP_C128, SKDSP_ERR_BADARG, "awgn_sigma: float32, complex64, float64 or complex128 rows (dtype code %d)", dtype);
    SK_CHECK(n >= 1 && nrow >= 0 && x_stride >= 0, SKDSP_ERR_BADARG, "awgn_sigma: rows of at least one element (n = %lld, nrow = %lld)", (long long)n, (long long)nrow);
    if (nrow == 0) return SKDSP_OK;
    SK_CHECK(x_dev && g_dev && sigma_dev, SKDSP_ERR_BADARG, "awgn_sigma: null pointer");
    API_BEGIN;
    void *scratch = nullptr;
    int rc = ws_reserve(3, symscale_scratch_bytes(n, nrow) + 256, &scratch);
    if (rc) return rc;
    if ((rc = symvar_launch(x_dev, x_stride, n, nrow, dtype, scratch, sigma_dev, ctx().stream))) return rc;
    return awgn_sigma_launch(mode, ns, p, var_w, nrow, g_dev, sigma_dev, ctx().stream);
}

// ---------------------------------------------------------------- OFDM
int skdsp_ofdm_tx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y_dev,
                           int64_t y_stride)
{
    return ofdm_tx_call(false, x_dev, x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, y_dev, y_stride);
}
int skdsp_ofdm_tx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y)
{
    const int64_t n_in = nsym * nf, n_out = npb == 1 ? 0 : (npb > 0 ? nsym + nsym / (npb - 1) + 1 : nsym) * (nc + (cp ? ncp : 0));
    return ofdm_tx_call(true, x, n_in, nsym, nrow, dtype, nf, nc, npb, cp, ncp, y, n_out);
}

int skdsp_ofdm_rx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                           const double *hht, void *z_dev, int64_t z_stride, void *h_dev)
{
    return ofdm_rx_call(false, x_dev, x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, alpha, hht, z_dev, z_stride, h_dev);
}
int skdsp_ofdm_rx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha, const double *hht, void *z, void *h)
{
    const int64_t n_in = nsym * (cp ? nc + ncp : nc), n_out = (nsym - (npb > 0 ? (nsym + npb - 1) / npb : 0)) * nf;
    return ofdm_rx_call(true, x, n_in, nsym, nrow, dtype, nf, nc, npb, cp, ncp, alpha, hht, z, n_out, h);
}

int skdsp_ofdm_equalize_rows_dev(const void *z_dev, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht,
                                 void *out_dev, int64_t out_stride, void *h_dev)
{
    return ofdm_equalize_call(false, z_dev, z_stride, nsym, nrow, dtype, nf, npb, alpha, hht, out_dev, out_stride, h_dev);
}
int skdsp_ofdm_equalize_rows(const void *z, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht, void *out, void *h)
{
    const int64_t n_in = nsym * nf, n_out = npb < 2 ? 0 : (nsym - (nsym + npb - 1) / npb) * nf;
    return ofdm_equalize_call(true, z, n_in, nsym, nrow, dtype, nf, npb, alpha, hht, out, n_out, h);
}

// ---------------------------------------------------------------- symbol-error tools
int skdsp_lag_corr_len(int64_t len, int64_t n_lags, int64_t *n_out, int64_t *first_lag)
{
    SK_CHECK(n_out && first_lag, SKDSP_ERR_BADARG, "lag_corr_len: null pointer");
    return lagcorr_check(len, n_lags, 0, 0, 0, n_out, first_lag);
}

int skdsp_lag_corr_dev(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, void *r_dev, double *e_dev)
{
    return lag_corr_call(false, a_dev, a_dtype, b_dev, b_dtype, len, n_lags, quant_levels, nullptr, r_dev, e_dev);
}
int skdsp_lag_corr(const void *a, int a_dtype, const void *b, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, int64_t *lags, void *r, double *e)
{
    return lag_corr_call(true, a, a_dtype, b, b_dtype, len, n_lags, quant_levels, lags, r, e);
}

int skdsp_sym_count_rows_dev(const void *tx_dev, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x_dev, int x_dtype, int64_t x_stride, int64_t start,
                             int64_t step, int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts_dev)
{
    return sym_count_call(false, tx_dev, tx_dtype, tx_stride, t0, x_dev, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, counts_dev);
}
int skdsp_sym_count_rows(const void *tx, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                         int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts)
{
    return sym_count_call(true, tx, tx_dtype, tx_stride, t0, x, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, counts);
}

// ---------------------------------------------------------------- pulse shaping and matched filtering over rows
// (pulse_create touches no device: the taps are uploaded by the first launch)
int skdsp_pulse_create(const double *b, int ntaps, int dtype, skdsp_handle *out) { return create_into("pulse", out, pulse_create, b, ntaps, dtype); }

int skdsp_pulse_mf_out_len(int64_t n, int64_t start, int64_t step, int64_t *n_out) { return pulse_mf_out_len(n, start, step, n_out); }

int skdsp_pulse_shape_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int ns, const double *scale, void *y_dev, int64_t y_stride)
{
    return pulse_shape_call(false, h, x_dev, n, nrow, x_stride, ns, scale, y_dev, y_stride);
}
int skdsp_pulse_shape_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int ns, const double *scale, void *y)
{
    return pulse_shape_call(true, h, x, n, nrow, n, ns, scale, y, n * ns);
}

int skdsp_pulse_mf_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, void *y_dev, int64_t y_stride)
{
    return pulse_mf_call(false, h, x_dev, n, nrow, x_stride, start, step, y_dev, y_stride);
}
int skdsp_pulse_mf_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int64_t start, int64_t step, void *y)
{
    return pulse_mf_call(true, h, x, n, nrow, n, start, step, y, 0);
}

// ---------------------------------------------------------------- carrier phase tracking and its impairment helpers over rows
int skdsp_carrier_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop,
                           double k1, double k2, const double *gains_dev, const double *r_dev, double inv_sqrt2, const double *tab_re, const double *tab_im, int outputs,
                           void *z_dev, void *a_dev, double *e_dev, double *t_dev, int64_t y_stride)
{
    return carrier_call(false, x_dev, n, nrow, x_stride, start, step, dtype, family, mod, type, open_loop, k1, k2, gains_dev, r_dev, 0.0, inv_sqrt2, tab_re, tab_im, outputs, z_dev,
                        a_dev, e_dev, t_dev, y_stride);
}
int skdsp_carrier_rows(const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, int dtype, int family, int mod, int type, int open_loop, double k1,
                       double k2, const double *gains, double qam_c, double inv_sqrt2, const double *tab_re, const double *tab_im, int outputs, void *z, void *a, double *e,
                       double *t)
{
    return carrier_call(true, x, n, nrow, x_stride, start, step, dtype, family, mod, type, open_loop, k1, k2, gains, nullptr, qam_c, inv_sqrt2, tab_re, tab_im, outputs, z, a, e, t, n);
}

int skdsp_time_step_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, int64_t t_step, const int64_t *t_steps_dev,
                             void *y_dev, int64_t n_out, int64_t y_stride)
{
    return impair_call(false, 0, x_dev, n, nrow, x_stride, dtype, ns, n_step, t_step, t_steps_dev, 1.0, 0.0, nullptr, y_dev, n_out, y_stride);
}
int skdsp_phase_step_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int dtype, int64_t ns, int64_t n_step, double f_re, double f_im,
                              const double *factors_dev, void *y_dev, int64_t y_stride)
{
    return impair_call(false, 1, x_dev, n, nrow, x_stride, dtype, ns, n_step, 0, nullptr, f_re, f_im, factors_dev, y_dev, ns >= 1 ? (n + ns - 1) / ns : 0, y_stride);
}

// ---------------------------------------------------------------- symbol timing recovery over rows
int skdsp_nda_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2,
                       const double *gains_dev, const double *rot, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *zz_dev,
                       double *e_tau_dev, int64_t *counts_dev, int64_t y_stride)
{
    return nda_call(false, x_dev, n, nrow, x_stride, start, dtype, ns, L, iord, k1, k2, gains_dev, rot, inv_ns, inv_len, k_eps, outputs, normalize, cap, zz_dev, e_tau_dev, counts_dev,
                    y_stride);
}
int skdsp_nda_rows(const void *x, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int dtype, int ns, int L, int iord, double k1, double k2, const double *gains,
                   const double *rot, double inv_ns, double inv_len, double k_eps, int outputs, int normalize, int64_t cap, void *zz, double *e_tau, int64_t *counts)
{
    return nda_call(true, x, n, nrow, x_stride, start, dtype, ns, L, iord, k1, k2, gains, rot, inv_ns, inv_len, k_eps, outputs, normalize, cap, zz, e_tau, counts, cap);
}

}  // extern "C"
