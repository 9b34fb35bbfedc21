// capi.hip -- the one-call wrappers of the extern "C" boundary of libskdsp_hip.so (see include/skdsp.h): FIR bank,
// resamplers, Farrow resampler, Welch primitive, Viterbi decoder, block codes, the FEC chain around the decoder, Gray symbol mapping.  The runtime is runtime.hip, the host-pointer chunk pipeline
// host_pipe.hip, FIR / IIR dispatch fir_api.hip / iir_api.hip.
#include "api_internal.hpp"

using namespace skdsp;

extern "C" {

// FIR bank (fir_bank.hip): argument errors need no device
int skdsp_fir_bank_create(const void *taps, int ntaps, int taps_complex, const int64_t *shifts, int nbands, int period, int dtype,
                          skdsp_handle *out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "fir_bank_create: null out");
    HandleBase *h = nullptr;
    int rc = fir_bank_create(taps, ntaps, taps_complex, shifts, nbands, period, dtype, &h);
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
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
int skdsp_upsample_dev(const void *x_dev, int64_t n, int L, int dtype, double scale, void *y_dev)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "upsample: bad dtype %d", dtype);
    return upsample_launch(x_dev, n, L, dtype, scale, y_dev, ctx().stream);
}

int skdsp_downsample_dev(const void *x_dev, int64_t n, int M, int p, int dtype, void *y_dev)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "downsample: bad dtype %d", dtype);
    return downsample_launch(x_dev, n, M, p, dtype, y_dev, ctx().stream);
}

int skdsp_upsample(const void *x, int64_t n, int L, int dtype, void *y)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype) && n >= 0 && L >= 1, SKDSP_ERR_BADARG, "upsample: bad arguments");
    if (n == 0) return SKDSP_OK;
    const size_t esz = dtype_size(dtype);
    void *x_dev = nullptr, *y_dev = nullptr;
    int rc = stage_in(x, (size_t)n * esz, &x_dev);
    if (rc) return rc;
    if ((rc = ws_reserve(1, (size_t)n * L * esz + 256, &y_dev))) return rc;
    if ((rc = upsample_launch(x_dev, n, L, dtype, 1.0, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, (size_t)n * L * esz);
}

int skdsp_downsample(const void *x, int64_t n, int M, int p, int dtype, void *y)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype) && n >= 0 && M >= 1, SKDSP_ERR_BADARG, "downsample: bad arguments");
    SK_CHECK(p >= 0 && p < M, SKDSP_ERR_BADARG, "downsample: phase p=%d out of range for M=%d", p, M);
    const int64_t n_out = n / M;
    if (n_out == 0) return SKDSP_OK;
    const size_t esz = dtype_size(dtype);
    void *x_dev = nullptr, *y_dev = nullptr;
    int rc = stage_in(x, (size_t)n * esz, &x_dev);
    if (rc) return rc;
    if ((rc = ws_reserve(1, (size_t)n_out * esz + 256, &y_dev))) return rc;
    if ((rc = downsample_launch(x_dev, n, M, p, dtype, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, (size_t)n_out * esz);
}

// ---------------------------------------------------------------- Farrow resampler
int skdsp_farrow_len(int64_t n, double Ts_old, double Ts_new, int64_t *n_out) { return farrow_len(n, Ts_old, Ts_new, n_out); }

int skdsp_farrow_dev(const void *x_dev, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int64_t n0,
                     int64_t count, int wide, void *y_dev)
{
    API_BEGIN;
    return farrow_launch(x_dev, n, dtype, Ts_old, Ts_new, i_ord, alpha, n0, count, wide, y_dev, ctx().stream);
}

int skdsp_farrow(const void *x, int64_t n, int dtype, double Ts_old, double Ts_new, int i_ord, double alpha, int wide, void *y)
{
    API_BEGIN;
    SK_CHECK(dtype_valid(dtype) && n >= 0, SKDSP_ERR_BADARG, "farrow: bad arguments");
    SK_CHECK(i_ord >= 1 && i_ord <= 3, SKDSP_ERR_BADARG, "farrow: i_ord must be 1, 2 or 3 (got %d)", i_ord);
    int64_t n_out = 0;
    int rc = farrow_len(n, Ts_old, Ts_new, &n_out);
    if (rc || n_out == 0) return rc;
    const size_t esz_out = dtype_size(dtype) * (!dtype_double(dtype) && (wide & SKDSP_FARROW_WIDE) ? 2 : 1);
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = stage_in(x, (size_t)n * dtype_size(dtype), &x_dev))) return rc;
    if ((rc = ws_reserve(1, (size_t)n_out * esz_out + 256, &y_dev))) return rc;
    if ((rc = farrow_launch(x_dev, n, dtype, Ts_old, Ts_new, i_ord, alpha, 0, n_out, wide, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, (size_t)n_out * esz_out);
}

// ---------------------------------------------------------------- Welch primitive (sigsys.psd, my_psd, simple_sa)
int skdsp_psd_dev(const void *x_dev, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg,
                  double *S_dev)
{
    int rc = psd_check(n, dtype, window, ns, n_fft, step, nseg);   // (argument errors need no device)
    if (rc) return rc;
    API_BEGIN;
    return psd_launch(x_dev, n, dtype, window, ns, n_fft, step, nseg, S_dev, ctx().stream);
}

int skdsp_psd(const void *x, int64_t n, int dtype, const double *window, int ns, int n_fft, int64_t step, int64_t nseg, double *S)
{
    int rc = psd_check(n, dtype, window, ns, n_fft, step, nseg);
    if (rc) return rc;
    SK_CHECK(x && S, SKDSP_ERR_BADARG, "psd: null pointer");
    API_BEGIN;
    const int64_t used = (nseg - 1) * step + ns;   // samples behind the last segment are not even copied
    void *x_dev = nullptr, *S_dev = nullptr;
    if ((rc = stage_in(x, (size_t)used * dtype_size(dtype), &x_dev))) return rc;
    if ((rc = ws_reserve(1, (size_t)n_fft * sizeof(double) + 256, &S_dev))) return rc;
    if ((rc = psd_launch(x_dev, used, dtype, window, ns, n_fft, step, nseg, (double *)S_dev, ctx().stream))) return rc;
    return stage_out(S, S_dev, (size_t)n_fft * sizeof(double));
}

// ---------------------------------------------------------------- Viterbi decoder (fec_conv.FECConv.viterbi_decoder)
int skdsp_viterbi_create(const char *const *polys, int npoly, int depth, skdsp_handle *out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "viterbi_create: null out");
    HandleBase *h = nullptr;
    int rc = viterbi_create(polys, npoly, depth, &h);
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
}

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

static int viterbi_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y_dev, int stateful)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_VITERBI);
    SK_CHECK(h, SKDSP_ERR_BADARG, "viterbi: not a Viterbi handle");
    int rc = viterbi_check(h, n, nrow, xtype, metric, quant_level, stateful);   // (argument errors need no device)
    if (rc) return rc;
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    return viterbi_launch(h, x_dev, n, nrow, xtype, metric, quant_level, y_dev, stateful, ctx().stream);
}

static int viterbi_host(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y, int stateful)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_VITERBI);
    SK_CHECK(h, SKDSP_ERR_BADARG, "viterbi: not a Viterbi handle");
    int rc = viterbi_check(h, n, nrow, xtype, metric, quant_level, stateful);
    if (rc) return rc;
    SK_CHECK(x, SKDSP_ERR_BADARG, "viterbi: null pointer");
    int64_t n_out = 0;
    if ((rc = viterbi_out_len(h, n, &n_out))) return rc;
    SK_CHECK(y || n_out == 0, SKDSP_ERR_BADARG, "viterbi: null pointer");
    if (!stateful && n_out == 0) return SKDSP_OK;
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = xtype == 0 ? 1 : xtype == 1 ? 2 : 8;
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = stage_in(x, (size_t)n * (size_t)nrow * esz, &x_dev))) return rc;
    if ((rc = ws_reserve(1, (size_t)n_out * (size_t)nrow + 256, &y_dev))) return rc;
    if ((rc = viterbi_launch(h, x_dev, n, nrow, xtype, metric, quant_level, (uint8_t *)y_dev, stateful, ctx().stream))) return rc;
    if (n_out == 0) return sync_checked();
    return stage_out(y, y_dev, (size_t)n_out * (size_t)nrow);
}

int skdsp_viterbi_decode(skdsp_handle h, const void *x, int64_t n, int xtype, int metric, int quant_level, uint8_t *y)
{
    return viterbi_host(h, x, n, 1, xtype, metric, quant_level, y, 1);
}

int skdsp_viterbi_decode_dev(skdsp_handle h, const void *x_dev, int64_t n, int xtype, int metric, int quant_level, uint8_t *y_dev)
{
    return viterbi_dev(h, x_dev, n, 1, xtype, metric, quant_level, y_dev, 1);
}

int skdsp_viterbi_decode_rows(skdsp_handle h, const void *x, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y)
{
    return viterbi_host(h, x, n, nrow, xtype, metric, quant_level, y, 0);
}

int skdsp_viterbi_decode_rows_dev(skdsp_handle h, const void *x_dev, int64_t n, int64_t nrow, int xtype, int metric, int quant_level, uint8_t *y_dev)
{
    return viterbi_dev(h, x_dev, n, nrow, xtype, metric, quant_level, y_dev, 0);
}

// ---------------------------------------------------------------- block codes (fec_block.FECHamming, fec_block.FECCyclic)
int skdsp_blockcode_create(int n, int k, const uint32_t *enc, const uint32_t *syn, const uint32_t *trap, skdsp_handle *out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "blockcode_create: null out");
    HandleBase *h = nullptr;
    int rc = blockcode_create(n, k, enc, syn, trap, &h);
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
}

static int blockcode_dev(skdsp_handle hh, int mode, const uint8_t *in_dev, int64_t nblocks, uint8_t *out_dev)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_BLOCKCODE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "blockcode: not a block code handle");
    int rc = blockcode_check(h, nblocks);   // (argument errors need no device)
    if (rc || nblocks == 0) return rc;
    SK_CHECK(in_dev && out_dev, SKDSP_ERR_BADARG, "blockcode: null pointer");
    API_BEGIN;
    std::lock_guard<std::mutex> lk(h->mu);
    return blockcode_launch(h, mode, in_dev, nblocks, out_dev, ctx().stream);
}

static int blockcode_host(skdsp_handle hh, int mode, const uint8_t *in, int64_t nblocks, uint8_t *out)
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
    const size_t bytes_in = (size_t)nblocks * (size_t)(mode == 0 ? k : n), bytes_out = (size_t)nblocks * (size_t)(mode == 0 ? n : k);
    void *in_dev = nullptr, *out_dev = nullptr;
    if ((rc = stage_in(in, bytes_in, &in_dev))) return rc;
    if ((rc = ws_reserve(1, bytes_out + 256, &out_dev))) return rc;
    if ((rc = blockcode_launch(h, mode, (const uint8_t *)in_dev, nblocks, (uint8_t *)out_dev, ctx().stream))) return rc;
    return stage_out(out, out_dev, bytes_out);
}

int skdsp_blockcode_encode(skdsp_handle h, const uint8_t *bits, int64_t nblocks, uint8_t *code) { return blockcode_host(h, 0, bits, nblocks, code); }
int skdsp_blockcode_encode_dev(skdsp_handle h, const uint8_t *bits_dev, int64_t nblocks, uint8_t *code_dev) { return blockcode_dev(h, 0, bits_dev, nblocks, code_dev); }
int skdsp_blockcode_decode(skdsp_handle h, const uint8_t *code, int64_t nblocks, uint8_t *bits) { return blockcode_host(h, 1, code, nblocks, bits); }
int skdsp_blockcode_decode_dev(skdsp_handle h, const uint8_t *code_dev, int64_t nblocks, uint8_t *bits_dev) { return blockcode_dev(h, 1, code_dev, nblocks, bits_dev); }

// ---------------------------------------------------------------- the FEC chain around the decoder (FECConv.conv_encoder / puncture / depuncture, digitalcom.bit_errors)
int skdsp_convcode_create(const char *const *polys, int npoly, skdsp_handle *out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "convcode_create: null out");
    HandleBase *h = nullptr;
    int rc = convcode_create(polys, npoly, &h);
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
}

int skdsp_convcode_encode_rows_dev(skdsp_handle hh, const uint8_t *bits_dev, int64_t n, int64_t nrow, const uint8_t *states_in_dev, int64_t nstates_in,
                                   uint8_t *code_dev, uint8_t *states_out_dev)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_CONVCODE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "convcode: not a convolutional code handle");
    int rc = convcode_check(h, n, nrow, nstates_in);   // (argument errors need no device)
    if (rc || nrow == 0) return rc;
    SK_CHECK(nstates_in == 0 || states_in_dev, SKDSP_ERR_BADARG, "convcode: null initial states");
    SK_CHECK(n == 0 || (bits_dev && code_dev), SKDSP_ERR_BADARG, "convcode: null pointer");
    if (n == 0 && !states_out_dev) return SKDSP_OK;
    API_BEGIN;
    return convcode_launch(h, bits_dev, n, nrow, states_in_dev, nstates_in, code_dev, states_out_dev, ctx().stream);
}

int skdsp_convcode_encode_rows(skdsp_handle hh, const uint8_t *bits, int64_t n, int64_t nrow, const uint8_t *states_in, int64_t nstates_in, uint8_t *code,
                               uint8_t *states_out)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_CONVCODE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "convcode: not a convolutional code handle");
    int rc = convcode_check(h, n, nrow, nstates_in);
    if (rc || nrow == 0) return rc;
    SK_CHECK(nstates_in == 0 || states_in, SKDSP_ERR_BADARG, "convcode: null initial states");
    int K = 0, R = 0;
    convcode_sizes(h, &K, &R);
    for (int64_t r = 0; r < nstates_in; ++r)
        SK_CHECK(states_in[r] < (1 << (K - 1)), SKDSP_ERR_BADARG, "convcode: state %d of row %lld does not fit the %d state bits", (int)states_in[r], (long long)r, K - 1);
    if (n == 0) {   // nothing to encode: the states pass through
        for (int64_t r = 0; states_out && r < nrow; ++r) states_out[r] = nstates_in == 0 ? 0 : states_in[nstates_in == 1 ? 0 : r];
        return SKDSP_OK;
    }
    SK_CHECK(bits && code, SKDSP_ERR_BADARG, "convcode: null pointer");
    API_BEGIN;
    // workspace 0: the bits; workspace 1: the code bits, then the states in (nrow bytes) and out (nrow bytes), each from a 256-byte boundary
    const size_t nbits = (size_t)n * (size_t)nrow, ncode = nbits * (size_t)R, st_off = round_up(ncode, 256), st_bytes = round_up((size_t)nrow, 256);
    void *bits_dev = nullptr, *out_dev = nullptr;
    if ((rc = stage_in(bits, nbits, &bits_dev))) return rc;
    if ((rc = ws_reserve(1, st_off + 2 * st_bytes + 256, &out_dev))) return rc;
    uint8_t *code_dev = (uint8_t *)out_dev, *sin_dev = code_dev + st_off, *sout_dev = sin_dev + st_bytes;
    if (nstates_in) SK_HIP(hipMemcpyAsync(sin_dev, states_in, (size_t)nstates_in, hipMemcpyHostToDevice, ctx().stream));
    if ((rc = convcode_launch(h, (const uint8_t *)bits_dev, n, nrow, sin_dev, nstates_in, code_dev, states_out ? sout_dev : nullptr, ctx().stream))) return rc;
    if (states_out) SK_HIP(hipMemcpyAsync(states_out, sout_dev, (size_t)nrow, hipMemcpyDeviceToHost, ctx().stream));
    return stage_out(code, code_dev, ncode);
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

static int gather_dev(int dep, const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y_dev)
{
    int64_t n_out = 0;
    int rc = gather_check(dep, n, nrow, elem_bytes, mask1, mask2, L_pp, &n_out);   // (argument errors need no device)
    if (rc) return rc;
    SK_CHECK(!dep || erase, SKDSP_ERR_BADARG, "depuncture: null erase value");
    if (nrow == 0 || n_out == 0) return SKDSP_OK;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "%s: null pointer", dep ? "depuncture" : "puncture");
    SK_CHECK(elem_aligned(x_dev, y_dev, elem_bytes), SKDSP_ERR_BADARG, "%s: the pointers must be aligned to the element", dep ? "depuncture" : "puncture");
    API_BEGIN;
    return gather_launch(dep, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y_dev, ctx().stream);
}

static int gather_host(int dep, const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y)
{
    int64_t n_out = 0;
    int rc = gather_check(dep, n, nrow, elem_bytes, mask1, mask2, L_pp, &n_out);
    if (rc) return rc;
    SK_CHECK(!dep || erase, SKDSP_ERR_BADARG, "depuncture: null erase value");
    if (nrow == 0 || n_out == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "%s: null pointer", dep ? "depuncture" : "puncture");
    API_BEGIN;
    const size_t bytes_in = (size_t)n * (size_t)nrow * (size_t)elem_bytes, bytes_out = (size_t)n_out * (size_t)nrow * (size_t)elem_bytes;
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = stage_in(x, bytes_in, &x_dev))) return rc;
    if ((rc = ws_reserve(1, bytes_out + 256, &y_dev))) return rc;
    if ((rc = gather_launch(dep, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, bytes_out);
}

int skdsp_puncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y)
{
    return gather_host(0, x, n, nrow, elem_bytes, mask1, mask2, L_pp, nullptr, y);
}
int skdsp_puncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, void *y_dev)
{
    return gather_dev(0, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, nullptr, y_dev);
}
int skdsp_depuncture_rows(const void *x, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y)
{
    return gather_host(1, x, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y);
}
int skdsp_depuncture_rows_dev(const void *x_dev, int64_t n, int64_t nrow, int elem_bytes, uint64_t mask1, uint64_t mask2, int L_pp, const void *erase, void *y_dev)
{
    return gather_dev(1, x_dev, n, nrow, elem_bytes, mask1, mask2, L_pp, erase, y_dev);
}

int skdsp_bit_count_rows_dev(const uint8_t *tx_dev, int64_t tx_stride, const uint8_t *rx_dev, int64_t rx_stride, int64_t n, int64_t nrow, int invert,
                             int64_t *counts_dev)
{
    int rc = bitcount_check(tx_stride, rx_stride, n, nrow);   // (argument errors need no device)
    if (rc || nrow == 0) return rc;
    SK_CHECK(counts_dev && ((uintptr_t)counts_dev & 7) == 0, SKDSP_ERR_BADARG, "bit_count: the counts must be an 8-byte aligned pointer");
    SK_CHECK(n == 0 || (tx_dev && rx_dev), SKDSP_ERR_BADARG, "bit_count: null pointer");
    API_BEGIN;
    return bitcount_launch(tx_dev, tx_stride, rx_dev, rx_stride, n, nrow, invert, counts_dev, ctx().stream);
}

// host form: both streams are copied whole -- (nrow - 1) stride + n bytes each
int skdsp_bit_count_rows(const uint8_t *tx, int64_t tx_stride, const uint8_t *rx, int64_t rx_stride, int64_t n, int64_t nrow, int invert, int64_t *counts)
{
    int rc = bitcount_check(tx_stride, rx_stride, n, nrow);
    if (rc || nrow == 0) return rc;
    SK_CHECK(counts, SKDSP_ERR_BADARG, "bit_count: null counts");
    if (n == 0) {
        for (int64_t r = 0; r < nrow; ++r) counts[r] = 0;
        return SKDSP_OK;
    }
    SK_CHECK(tx && rx, SKDSP_ERR_BADARG, "bit_count: null pointer");
    API_BEGIN;
    const size_t tx_bytes = (size_t)((nrow - 1) * tx_stride + n), rx_bytes = (size_t)((nrow - 1) * rx_stride + n), cnt_off = round_up(rx_bytes, 256);
    void *tx_dev = nullptr, *rx_dev = nullptr;
    if ((rc = ws_reserve(1, cnt_off + (size_t)nrow * sizeof(int64_t) + 256, &rx_dev))) return rc;
    if ((rc = stage_in(tx, tx_bytes, &tx_dev))) return rc;
    SK_HIP(hipMemcpyAsync(rx_dev, rx, rx_bytes, hipMemcpyHostToDevice, ctx().stream));
    int64_t *counts_dev = reinterpret_cast<int64_t *>((char *)rx_dev + cnt_off);
    if ((rc = bitcount_launch((const uint8_t *)tx_dev, tx_stride, (const uint8_t *)rx_dev, rx_stride, n, nrow, invert, counts_dev, ctx().stream))) return rc;
    return stage_out(counts, counts_dev, (size_t)nrow * sizeof(int64_t));
}

// ---------------------------------------------------------------- Gray symbol mapping (symmap.hip): qam_gray_encode_bb / mpsk_gray_encode_bb's symbols, qam_gray_decode / mpsk_gray_decode
int skdsp_gray_map_rows_dev(const uint8_t *bits_dev, int64_t bits_stride, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab,
                            int dtype, void *y_dev, int64_t y_stride)
{
    int rc = symmap_check(kind, mod, n, nrow, dtype, bits_stride, y_stride);   // (argument errors need no device)
    if (rc) return rc;
    SK_CHECK(tab_re, SKDSP_ERR_BADARG, "gray_map: null table");
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(bits_dev && y_dev, SKDSP_ERR_BADARG, "gray_map: null pointer");
    API_BEGIN;
    return symmap_launch(bits_dev, bits_stride, n, nrow, kind, mod, tab_re, tab_im, ntab, dtype, y_dev, y_stride, ctx().stream);
}

// host form: contiguous rows -- nrow x (bps n) bytes in, nrow x n points out
int skdsp_gray_map_rows(const uint8_t *bits, int64_t n, int64_t nrow, int kind, int mod, const double *tab_re, const double *tab_im, int ntab, int dtype, void *y)
{
    const int bps = sym_bits_per_symbol(kind, mod);
    int rc = symmap_check(kind, mod, n, nrow, dtype, bps * n, n);
    if (rc) return rc;
    SK_CHECK(tab_re, SKDSP_ERR_BADARG, "gray_map: null table");
    if (nrow == 0 || n == 0) return SKDSP_OK;
    SK_CHECK(bits && y, SKDSP_ERR_BADARG, "gray_map: null pointer");
    API_BEGIN;
    const size_t bytes_in = (size_t)bps * (size_t)n * (size_t)nrow, bytes_out = (size_t)n * (size_t)nrow * dtype_size(dtype);
    void *bits_dev = nullptr, *y_dev = nullptr;
    if ((rc = stage_in(bits, bytes_in, &bits_dev))) return rc;
    if ((rc = ws_reserve(1, bytes_out + 256, &y_dev))) return rc;
    if ((rc = symmap_launch((const uint8_t *)bits_dev, bps * n, n, nrow, kind, mod, tab_re, tab_im, ntab, dtype, y_dev, n, ctx().stream))) return rc;
    return stage_out(y, y_dev, bytes_out);
}

// the partial moments of a launch live in workspace 3 of the calling slot
int skdsp_qam_scale_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r_dev)
{
    int rc = symscale_check(mod, n, nrow, dtype, x_stride, start, step);   // (argument errors need no device)
    if (rc || nrow == 0) return rc;
    SK_CHECK(n >= 1, SKDSP_ERR_BADARG, "qam_scale: a row has no symbols");
    SK_CHECK(x_dev && r_dev, SKDSP_ERR_BADARG, "qam_scale: null pointer");
    API_BEGIN;
    void *scratch = nullptr;
    if ((rc = ws_reserve(3, symscale_scratch_bytes(n, nrow) + 256, &scratch))) return rc;
    return symscale_launch(x_dev, x_stride, start, step, n, nrow, dtype, mod, c, scratch, r_dev, ctx().stream);
}

// host forms of the strided calls: the rows are copied whole -- (nrow - 1) x_stride + start + (n - 1) step + 1 elements
static size_t sym_span(int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow) { return (size_t)((nrow - 1) * x_stride + start + (n - 1) * step + 1); }

int skdsp_qam_scale_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double c, double *r)
{
    int rc = symscale_check(mod, n, nrow, dtype, x_stride, start, step);
    if (rc || nrow == 0) return rc;
    SK_CHECK(n >= 1, SKDSP_ERR_BADARG, "qam_scale: a row has no symbols");
    SK_CHECK(x && r, SKDSP_ERR_BADARG, "qam_scale: null pointer");
    API_BEGIN;
    void *x_dev = nullptr, *r_dev = nullptr, *scratch = nullptr;
    if ((rc = stage_in(x, sym_span(x_stride, start, step, n, nrow) * dtype_size(dtype), &x_dev))) return rc;
    if ((rc = ws_reserve(1, (size_t)nrow * sizeof(double) + 256, &r_dev))) return rc;
    if ((rc = ws_reserve(3, symscale_scratch_bytes(n, nrow) + 256, &scratch))) return rc;
    if ((rc = symscale_launch(x_dev, x_stride, start, step, n, nrow, dtype, mod, c, scratch, (double *)r_dev, ctx().stream))) return rc;
    return stage_out(r, r_dev, (size_t)nrow * sizeof(double));
}

int skdsp_qam_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r_dev,
                             uint8_t *bits_dev, int64_t bits_stride)
{
    int rc = symdemap_check(0, mod, n, nrow, dtype, x_stride, start, step, bits_stride);   // (argument errors need no device)
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x_dev && r_dev && bits_dev, SKDSP_ERR_BADARG, "qam_demap: null pointer");
    API_BEGIN;
    return symdemap_launch(x_dev, x_stride, start, step, n, nrow, dtype, 0, mod, r_dev, 1.0, 0.0, bits_dev, bits_stride, ctx().stream);
}

int skdsp_mpsk_demap_rows_dev(const void *x_dev, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                              uint8_t *bits_dev, int64_t bits_stride)
{
    int rc = symdemap_check(1, mod, n, nrow, dtype, x_stride, start, step, bits_stride);   // (argument errors need no device)
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x_dev && bits_dev, SKDSP_ERR_BADARG, "mpsk_demap: null pointer");
    API_BEGIN;
    return symdemap_launch(x_dev, x_stride, start, step, n, nrow, dtype, 1, mod, nullptr, rot_re, rot_im, bits_dev, bits_stride, ctx().stream);
}

// host form of both demappers: r: the rows' scales (QAM; HOST pointer), bits: nrow contiguous rows of bps n bytes
static int demap_host(int kind, const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r, double rot_re,
                      double rot_im, uint8_t *bits)
{
    const int bps = sym_bits_per_symbol(kind, mod);
    int rc = symdemap_check(kind, mod, n, nrow, dtype, x_stride, start, step, bps * n);
    if (rc || nrow == 0 || n == 0) return rc;
    SK_CHECK(x && bits && (kind || r), SKDSP_ERR_BADARG, "%s: null pointer", kind ? "mpsk_demap" : "qam_demap");
    API_BEGIN;
    const size_t bytes_out = (size_t)bps * (size_t)n * (size_t)nrow, r_off = round_up(bytes_out, 256);
    void *x_dev = nullptr, *out_dev = nullptr;
    if ((rc = stage_in(x, sym_span(x_stride, start, step, n, nrow) * dtype_size(dtype), &x_dev))) return rc;
    if ((rc = ws_reserve(1, r_off + (size_t)nrow * sizeof(double) + 256, &out_dev))) return rc;
    double *r_dev = reinterpret_cast<double *>((char *)out_dev + r_off);
    if (!kind) SK_HIP(hipMemcpyAsync(r_dev, r, (size_t)nrow * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    if ((rc = symdemap_launch(x_dev, x_stride, start, step, n, nrow, dtype, kind, mod, kind ? nullptr : r_dev, rot_re, rot_im, (uint8_t *)out_dev, bps * n, ctx().stream))) return rc;
    return stage_out(bits, out_dev, bytes_out);
}

int skdsp_qam_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, const double *r, uint8_t *bits)
{
    return demap_host(0, x, x_stride, start, step, n, nrow, dtype, mod, r, 1.0, 0.0, bits);
}
int skdsp_mpsk_demap_rows(const void *x, int64_t x_stride, int64_t start, int64_t step, int64_t n, int64_t nrow, int dtype, int mod, double rot_re, double rot_im,
                          uint8_t *bits)
{
    return demap_host(1, x, x_stride, start, step, n, nrow, dtype, mod, nullptr, rot_re, rot_im, bits);
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

// ---------------------------------------------------------------- OFDM (ofdm.hip): ofdm_tx / ofdm_rx / chan_est_equalize over rows
// the pilots, the estimates, the raw data rows and the channel table of a launch live in workspace 3 of the calling slot
int skdsp_ofdm_tx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y_dev,
                           int64_t y_stride)
{
    int rc = ofdm_tx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, x_stride, y_stride);   // (argument errors need no device)
    if (rc || nrow == 0) return rc;
    API_BEGIN;
    return ofdm_tx_launch(x_dev, x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, y_dev, y_stride, ctx().stream);
}

int skdsp_ofdm_tx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, void *y)
{
    const int64_t n_in = nsym * nf, n_out = npb == 1 ? 0 : (npb > 0 ? nsym + nsym / (npb - 1) + 1 : nsym) * (nc + (cp ? ncp : 0));
    int rc = ofdm_tx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, n_in, n_out);
    if (rc || nrow == 0) return rc;
    if (n_out == 0) return SKDSP_OK;
    SK_CHECK(y && (x || n_in == 0), SKDSP_ERR_BADARG, "ofdm_tx: null pointer");
    API_BEGIN;
    const size_t esz = dtype_size(dtype);
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = stage_in(x, (size_t)n_in * (size_t)nrow * esz, &x_dev))) return rc;
    if ((rc = ws_reserve(1, (size_t)n_out * (size_t)nrow * esz + 256, &y_dev))) return rc;
    if ((rc = ofdm_tx_launch(x_dev, n_in, nsym, nrow, dtype, nf, nc, npb, cp, ncp, y_dev, n_out, ctx().stream))) return rc;
    return stage_out(y, y_dev, (size_t)n_out * (size_t)nrow * esz);
}

int skdsp_ofdm_rx_rows_dev(const void *x_dev, int64_t x_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha,
                           const double *hht, void *z_dev, int64_t z_stride, void *h_dev)
{
    int rc = ofdm_rx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, hht != nullptr, x_stride, z_stride);   // (argument errors need no device)
    if (rc || nrow == 0 || nsym == 0) return rc;
    API_BEGIN;
    void *scratch = nullptr;
    if ((rc = ws_reserve(3, ofdm_scratch_bytes(nsym, nrow, nf), &scratch))) return rc;
    return ofdm_rx_launch(x_dev, x_stride, nsym, nrow, dtype, nf, nc, npb, cp, ncp, alpha, hht, scratch, z_dev, z_stride, h_dev, ctx().stream);
}

int skdsp_ofdm_rx_rows(const void *x, int64_t nsym, int64_t nrow, int dtype, int nf, int nc, int npb, int cp, int ncp, double alpha, const double *hht, void *z, void *h)
{
    const int64_t n_in = nsym * (cp ? nc + ncp : nc);
    const int64_t n_out = (nsym - (npb > 0 ? (nsym + npb - 1) / npb : 0)) * nf;
    int rc = ofdm_rx_check(nsym, nrow, dtype, nf, nc, npb, cp, ncp, hht != nullptr, n_in, n_out);
    if (rc || nrow == 0 || nsym == 0) return rc;
    SK_CHECK(x && (z || n_out == 0) && (h || npb <= 0), SKDSP_ERR_BADARG, "ofdm_rx: null pointer");
    API_BEGIN;
    const size_t esz = dtype_size(dtype), z_bytes = (size_t)n_out * (size_t)nrow * esz, h_off = round_up(z_bytes, 256), h_bytes = npb > 0 ? (size_t)nrow * nf * 16 : 0;
    void *x_dev = nullptr, *out_dev = nullptr, *scratch = nullptr;
    if ((rc = stage_in(x, (size_t)n_in * (size_t)nrow * esz, &x_dev))) return rc;
    if ((rc = ws_reserve(1, h_off + h_bytes + 256, &out_dev))) return rc;
    if ((rc = ws_reserve(3, ofdm_scratch_bytes(nsym, nrow, nf), &scratch))) return rc;
    void *h_dev = (char *)out_dev + h_off;
    if ((rc = ofdm_rx_launch(x_dev, n_in, nsym, nrow, dtype, nf, nc, npb, cp, ncp, alpha, hht, scratch, out_dev, n_out, h_dev, ctx().stream))) return rc;
    if (h_bytes && (rc = stage_out(h, h_dev, h_bytes))) return rc;
    return z_bytes ? stage_out(z, out_dev, z_bytes) : sync_checked();
}

int skdsp_ofdm_equalize_rows_dev(const void *z_dev, int64_t z_stride, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht,
                                 void *out_dev, int64_t out_stride, void *h_dev)
{
    int rc = ofdm_equalize_check(nsym, nrow, dtype, nf, npb, z_stride, out_stride);   // (argument errors need no device)
    if (rc || nrow == 0 || nsym == 0) return rc;
    API_BEGIN;
    void *scratch = nullptr;
    if ((rc = ws_reserve(3, ofdm_scratch_bytes(nsym, nrow, nf), &scratch))) return rc;
    return ofdm_equalize_launch(z_dev, z_stride, nsym, nrow, dtype, nf, npb, alpha, hht, scratch, out_dev, out_stride, h_dev, ctx().stream);
}

int skdsp_ofdm_equalize_rows(const void *z, int64_t nsym, int64_t nrow, int dtype, int nf, int npb, double alpha, const double *hht, void *out, void *h)
{
    const int64_t n_in = nsym * nf, n_out = npb < 2 ? 0 : (nsym - (nsym + npb - 1) / npb) * nf;
    int rc = ofdm_equalize_check(nsym, nrow, dtype, nf, npb, n_in, n_out);
    if (rc || nrow == 0 || nsym == 0) return rc;
    SK_CHECK(z && h && (out || n_out == 0), SKDSP_ERR_BADARG, "ofdm_equalize: null pointer");
    API_BEGIN;
    const size_t esz = dtype_size(dtype), o_bytes = (size_t)n_out * (size_t)nrow * esz, h_off = round_up(o_bytes, 256), h_bytes = (size_t)nrow * nf * 16;
    void *z_dev = nullptr, *out_dev = nullptr, *scratch = nullptr;
    if ((rc = stage_in(z, (size_t)n_in * (size_t)nrow * esz, &z_dev))) return rc;
    if ((rc = ws_reserve(1, h_off + h_bytes + 256, &out_dev))) return rc;
    if ((rc = ws_reserve(3, ofdm_scratch_bytes(nsym, nrow, nf), &scratch))) return rc;
    void *h_dev = (char *)out_dev + h_off;
    if ((rc = ofdm_equalize_launch(z_dev, n_in, nsym, nrow, dtype, nf, npb, alpha, hht, scratch, out_dev, n_out, h_dev, ctx().stream))) return rc;
    if ((rc = stage_out(h, h_dev, h_bytes))) return rc;
    return o_bytes ? stage_out(out, out_dev, o_bytes) : SKDSP_OK;
}

// ---------------------------------------------------------------- symbol-error tools (symerr.hip): xcorr / qam_sep / qpsk_bep / bpsk_bep
int skdsp_lag_corr_len(int64_t len, int64_t n_lags, int64_t *n_out, int64_t *first_lag)
{
    SK_CHECK(n_out && first_lag, SKDSP_ERR_BADARG, "lag_corr_len: null pointer");
    return lagcorr_check(len, n_lags, 0, 0, 0, n_out, first_lag);
}

// the partials of a launch live in workspace 3 of the calling slot
int skdsp_lag_corr_dev(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, void *r_dev, double *e_dev)
{
    int64_t nl = 0;
    int rc = lagcorr_check(len, n_lags, a_dtype, b_dtype, quant_levels, &nl, nullptr);   // (argument errors need no device)
    if (rc || nl == 0) return rc;
    SK_CHECK(a_dev && b_dev && r_dev && e_dev, SKDSP_ERR_BADARG, "lag_corr: null pointer");
    API_BEGIN;
    void *scratch = nullptr;
    if ((rc = ws_reserve(3, lagcorr_scratch_bytes(len, n_lags), &scratch))) return rc;
    return lagcorr_launch(a_dev, a_dtype, b_dev, b_dtype, len, n_lags, quant_levels, scratch, r_dev, e_dev, ctx().stream);
}

// host form: the first K elements of both streams are copied
int skdsp_lag_corr(const void *a, int a_dtype, const void *b, int b_dtype, int64_t len, int64_t n_lags, int quant_levels, int64_t *lags, void *r, double *e)
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
    const size_t a_bytes = (size_t)K * dtype_size(a_dtype), b_bytes = (size_t)K * dtype_size(b_dtype), r_off = round_up(b_bytes, 256), r_bytes = (size_t)nl * 16;
    const size_t e_off = r_off + round_up(r_bytes, 256);
    void *a_dev = nullptr, *b_dev = nullptr, *scratch = nullptr;
    if ((rc = ws_reserve(1, e_off + 256, &b_dev))) return rc;
    if ((rc = ws_reserve(3, lagcorr_scratch_bytes(len, n_lags), &scratch))) return rc;
    if ((rc = stage_in(a, a_bytes, &a_dev))) return rc;
    SK_HIP(hipMemcpyAsync(b_dev, b, b_bytes, hipMemcpyHostToDevice, ctx().stream));
    void *r_dev = (char *)b_dev + r_off;
    double *e_dev = reinterpret_cast<double *>((char *)b_dev + e_off);
    if ((rc = lagcorr_launch(a_dev, a_dtype, b_dev, b_dtype, len, n_lags, quant_levels, scratch, r_dev, e_dev, ctx().stream))) return rc;
    SK_HIP(hipMemcpyAsync(e, e_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    return stage_out(r, r_dev, r_bytes);
}

int skdsp_sym_count_rows_dev(const void *tx_dev, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x_dev, int x_dtype, int64_t x_stride, int64_t start,
                             int64_t step, int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts_dev)
{
    int rc = symcount_check(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase);   // (argument errors need no device)
    if (rc || nrow == 0) return rc;
    SK_CHECK(counts_dev && ((uintptr_t)counts_dev & 7) == 0, SKDSP_ERR_BADARG, "sym_count: the counts must be an 8-byte aligned pointer");
    SK_CHECK(n == 0 || (tx_dev && x_dev), SKDSP_ERR_BADARG, "sym_count: null pointer");
    API_BEGIN;
    return symcount_launch(tx_dev, tx_dtype, tx_stride, t0, x_dev, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, counts_dev, ctx().stream);
}

// host form: both arrays are copied whole -- through the last element a row reads
int skdsp_sym_count_rows(const void *tx, int tx_dtype, int64_t tx_stride, int64_t t0, const void *x, int x_dtype, int64_t x_stride, int64_t start, int64_t step,
                         int64_t r0, int64_t n, int64_t nrow, int mode, int levels, int kphase, int64_t *counts)
{
    int rc = symcount_check(tx_dtype, tx_stride, t0, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase);
    if (rc || nrow == 0) return rc;
    SK_CHECK(counts, SKDSP_ERR_BADARG, "sym_count: null counts");
    if (n == 0) {
        for (int64_t i = 0; i < 4 * nrow; ++i) counts[i] = 0;
        return SKDSP_OK;
    }
    SK_CHECK(tx && x, SKDSP_ERR_BADARG, "sym_count: null pointer");
    API_BEGIN;
    const size_t tx_bytes = (size_t)((nrow - 1) * tx_stride + t0 + n) * dtype_size(tx_dtype);
    const size_t x_bytes = (size_t)((nrow - 1) * x_stride + start + (r0 + n - 1) * step + 1) * dtype_size(x_dtype), cnt_off = round_up(x_bytes, 256);
    void *tx_dev = nullptr, *x_dev = nullptr;
    if ((rc = ws_reserve(1, cnt_off + (size_t)nrow * 4 * sizeof(int64_t) + 256, &x_dev))) return rc;
    if ((rc = stage_in(tx, tx_bytes, &tx_dev))) return rc;
    SK_HIP(hipMemcpyAsync(x_dev, x, x_bytes, hipMemcpyHostToDevice, ctx().stream));
    int64_t *counts_dev = reinterpret_cast<int64_t *>((char *)x_dev + cnt_off);
    if ((rc = symcount_launch(tx_dev, tx_dtype, tx_stride, t0, x_dev, x_dtype, x_stride, start, step, r0, n, nrow, mode, levels, kphase, counts_dev, ctx().stream))) return rc;
    return stage_out(counts, counts_dev, (size_t)nrow * 4 * sizeof(int64_t));
}

// ---------------------------------------------------------------- pulse shaping and matched filtering over rows (pulse.hip): sigsys.pulse_shape_rows / matched_filter_rows
int skdsp_pulse_create(const double *b, int ntaps, int dtype, skdsp_handle *out)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "pulse_create: null out");
    HandleBase *h = nullptr;
    int rc = pulse_create(b, ntaps, dtype, &h);   // (no device: the taps are uploaded by the first launch)
    if (rc) return rc;
    *out = h;
    return SKDSP_OK;
}

int skdsp_pulse_mf_out_len(int64_t n, int64_t start, int64_t step, int64_t *n_out) { return pulse_mf_out_len(n, start, step, n_out); }

int skdsp_pulse_shape_rows_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int ns, const double *scale, void *y_dev, int64_t y_stride)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_shape: not a pulse handle");
    int rc = pulse_shape_check(h, n, nrow, ns, x_stride, y_stride);   // (argument errors need no device)
    if (rc || n == 0 || nrow == 0) return rc;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "pulse_shape: null pointer");
    API_BEGIN;
    return pulse_shape_launch(h, x_dev, n, nrow, ns, x_stride, y_stride, scale != nullptr, scale ? *scale : 1.0, y_dev, ctx().stream);
}

// host form: rows contiguous in x (n each) and in y (n ns each)
int skdsp_pulse_shape_rows(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int ns, const double *scale, void *y)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_shape: not a pulse handle");
    int rc = pulse_shape_check(h, n, nrow, ns, n, n * ns);
    if (rc || n == 0 || nrow == 0) return rc;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "pulse_shape: null pointer");
    API_BEGIN;
    const size_t esz = dtype_size(h->dtype), y_bytes = (size_t)n * (size_t)ns * (size_t)nrow * esz;
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = ws_reserve(1, y_bytes + 256, &y_dev))) return rc;
    if ((rc = stage_in(x, (size_t)n * (size_t)nrow * esz, &x_dev))) return rc;
    if ((rc = pulse_shape_launch(h, x_dev, n, nrow, ns, n, n * ns, scale != nullptr, scale ? *scale : 1.0, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, y_bytes);
}

int skdsp_pulse_mf_rows_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t start, int64_t step, void *y_dev, int64_t y_stride)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_mf: not a pulse handle");
    int rc = pulse_mf_check(h, n, nrow, start, step, x_stride, y_stride);   // (argument errors need no device)
    if (rc || nrow == 0 || n <= start) return rc;
    SK_CHECK(x_dev && y_dev, SKDSP_ERR_BADARG, "pulse_mf: null pointer");
    API_BEGIN;
    return pulse_mf_launch(h, x_dev, n, nrow, start, step, x_stride, y_stride, y_dev, ctx().stream);
}

// host form: rows contiguous in x (n each) and in y (skdsp_pulse_mf_out_len each)
int skdsp_pulse_mf_rows(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, int64_t start, int64_t step, void *y)
{
    HandleBase *h = as_handle<HandleBase>(hh, H_PULSE);
    SK_CHECK(h, SKDSP_ERR_BADARG, "pulse_mf: not a pulse handle");
    int64_t n_out = 0;
    int rc = step >= 1 && step <= 64 ? pulse_mf_out_len(n, start, step, &n_out) : SKDSP_OK;   // (a step the kernel does not take: the check below says so)
    if (rc) return rc;
    rc = pulse_mf_check(h, n, nrow, start, step, n, n_out);
    if (rc || nrow == 0 || n_out == 0) return rc;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "pulse_mf: null pointer");
    API_BEGIN;
    const size_t esz = dtype_size(h->dtype), y_bytes = (size_t)n_out * (size_t)nrow * esz;
    void *x_dev = nullptr, *y_dev = nullptr;
    if ((rc = ws_reserve(1, y_bytes + 256, &y_dev))) return rc;
    if ((rc = stage_in(x, (size_t)n * (size_t)nrow * esz, &x_dev))) return rc;
    if ((rc = pulse_mf_launch(h, x_dev, n, nrow, start, step, n, n_out, y_dev, ctx().stream))) return rc;
    return stage_out(y, y_dev, y_bytes);
}

}  // extern "C"
