"""fec_conv.FECConv of scikit-dsp-comm (fec_conv.py:117-712) with the Viterbi decoder on the GPU (csrc/viterbi.hip).

    viterbi_decoder        one stream, bit for bit the reference's output -- including its statefulness: the reference object
                           keeps its trellis (metrics and histories) from call to call, so a second call continues the first
    viterbi_decoder_rows   beyond the reference: every row an independent frame decoded from rest, all rows in one launch
    viterbi_decoder_host   the same decoder in float64 NumPy, vectorised over the states: the yardstick of the GPU tests
                           (viterbi_decoder_rows_host: the same over many rows at once)
    reset                  beyond the reference: back to rest
    conv_encoder, puncture, depuncture   NumPy on the host by design (like sigsys.cic), bit-exact with the reference
    conv_encoder_rows, puncture_rows, depuncture_rows   beyond the reference: the same three over the rows of a frame set on the GPU
                           (csrc/convcode.hip), each row equal to the 1-D method's result; with digitalcom.bit_errors(_rows) the BER loop
                           encode -> puncture -> channel -> depuncture -> viterbi_decoder_rows -> count runs on device kernels throughout

The decoder is a register-exchange decoder: each of the 2^(K-1) states carries its last Depth decided bits; a step copies the
surviving predecessor's history (d1 <= d2 keeps the even predecessor) and shifts the state's input bit in; from step Depth - 1 on
the oldest bit of the FIRST state with the minimum metric is emitted.  State numbers are the reference's state strings read as
binary (newest bit first): state m is entered from 2 (m mod Ns/2) and the state after it under input bit m >> (K - 2).

Deliberate differences from the reference (tests/golden/g19_conventions.json: deliberate_differences): no paths.cumulative_metric;
non-finite soft / unquant input, 2-D input, |int(x)| > 4095 or quant_level outside 0 ... 12 for soft, and a change of metric family
on an object that is not at rest raise ValueError; lists and tuples are accepted; K = 3 ... 9 and Depth = 1 ... 128 only.
"""
import warnings
from fractions import Fraction
from logging import getLogger

import numpy as np

from . import _ffi

log = getLogger(__name__)

MAX_DEPTH = 128
SOFT_MAX_ABS = 4095
SOFT_MAX_QUANT = 12
_METRICS = {"hard": 0, "soft": 1, "unquant": 2}


def binary(num, length=8):
    """Format an integer to binary without the leading '0b'"""
    return format(num, '0{}b'.format(length))


class FECConv(object):
    """Rate 1/2 or 1/3 convolutional code: G is a tuple of two or three strings of K binary digits, Depth the decision depth."""

    def __init__(self, G=('111', '101'), Depth=10):
        self.G_polys = G
        self.constraint_length = len(self.G_polys[0])
        self.Nstates = 2 ** (self.constraint_length - 1)
        self.decision_depth = Depth
        self.rate = Fraction(1, len(G))
        if len(G) == 2 or len(G) == 3:
            log.info('Rate %s Object' % (self.rate))
        else:
            warnings.warn('Invalid rate. Use Rate 1/2 or 1/3 only')
            raise ValueError('Invalid rate. Use Rate 1/2 or 1/3 only')
        K, R = self.constraint_length, len(G)
        if not 3 <= K <= 9:
            raise ValueError("FECConv: polynomials of K = 3 ... 9 digits are served (got K = %d)" % K)
        if any(len(g) != K or set(g) - {'0', '1'} for g in G):
            raise ValueError("FECConv: the polynomials must be strings of 0 and 1 of the same length")
        if int(Depth) != Depth or not 1 <= Depth <= MAX_DEPTH:
            raise ValueError("FECConv: Depth must be 1 ... %d (got %r)" % (MAX_DEPTH, Depth))
        self.decision_depth = int(Depth)
        # polynomial j as a mask over the register [input, state]; the reference's rate-1/2 encoder feeds the input into both
        # outputs whatever the first digits are, its rate-1/3 encoder honours them (fec_conv.py:517-553)
        self._taps = np.array([[int(c) for c in g] for g in G], dtype=np.int64)
        if R == 2:
            self._taps[:, 0] = 1
        masks = [int("".join(str(v) for v in row), 2) for row in self._taps]
        Ns = self.Nstates
        m = np.arange(Ns)
        self._p0 = 2 * (m % (Ns // 2))
        self._p1 = self._p0 + 1
        self._u = (m >> (K - 2)).astype(np.uint64)

        def word(p):
            reg = (self._u.astype(np.int64) << (K - 1)) | p
            w = np.zeros(Ns, dtype=np.int64)
            for mask in masks:
                w = (w << 1) | np.array([bin(int(v) & mask).count("1") & 1 for v in reg])
            return w
        self._bits1, self._bits2 = word(self._p0), word(self._p1)
        self._kern = None
        self._enc_kern = None
        self._host_reset()

    # ------------------------------------------------------------------ state
    def _host_reset(self):
        self._host_cm = np.zeros(self.Nstates)
        self._host_hist = np.zeros((self.Nstates, (self.decision_depth + 63) // 64), dtype=np.uint64)

    def _kernel(self):
        if self._kern is None:
            self._kern = _ffi.ViterbiKernel(self.G_polys, self.decision_depth)
        return self._kern

    def reset(self):
        """Beyond the reference: the decoder (viterbi_decoder's device state and viterbi_decoder_host's) back to rest."""
        self._host_reset()
        if self._kern is not None:
            self._kern.reset()

    # ------------------------------------------------------------------ the received values
    def _received(self, x, metric_type, quant_level, ndim):
        """x as the decoders read it: validated, (int64 0 / 1 | truncated float64 | float64), by the reference's rules where it has any"""
        if metric_type not in _METRICS:
            warnings.warn('Invalid metric type specified')
            raise ValueError('Invalid metric type specified. Use soft, hard, or unquant')
        x = np.asarray(x)
        if x.ndim != ndim:
            if ndim == 1:
                raise ValueError("viterbi_decoder takes one stream of received values (one-dimensional); viterbi_decoder_rows decodes "
                                 "the rows of a 2-D array as independent frames")
            raise ValueError("viterbi_decoder_rows takes a 2-D array, one frame per row")
        nval = x.shape[-1]
        if nval < self.decision_depth:
            raise ValueError("fewer received values (%d) than the decision depth (%d)" % (nval, self.decision_depth))
        if metric_type == 'hard':
            if not np.issubdtype(x.dtype, np.integer):
                raise ValueError('Decoder inputs must be integers on [0,1] for hard decisions')
            if x.max() > 1 or x.min() < 0:
                raise ValueError('Integer bit values must be 0 or 1')
            return x.astype(np.int64)
        if nval % self.rate.denominator:
            raise IndexError("%d received values are no multiple of the %d per symbol" % (nval, self.rate.denominator))
        x = x.astype(np.float64)
        if not np.all(np.isfinite(x)):
            raise ValueError("viterbi_decoder: non-finite received value")
        if metric_type == 'soft':
            if int(quant_level) != quant_level or not 0 <= quant_level <= SOFT_MAX_QUANT:
                raise ValueError("viterbi_decoder: quant_level must be 0 ... %d (got %r)" % (SOFT_MAX_QUANT, quant_level))
            x = np.trunc(x)   # the reference takes int() of every value: toward zero, so a 3.5 erasure counts as 3
            if np.max(np.abs(x)) > SOFT_MAX_ABS:
                raise ValueError("viterbi_decoder: soft values beyond +-%d" % SOFT_MAX_ABS)
        return x

    # ------------------------------------------------------------------ GPU
    def viterbi_decoder(self, x, metric_type='soft', quant_level=3):
        """Decoded 0. / 1. bits (float64), one per symbol from symbol Depth - 1 on, continuing from where the previous call on this
        object ended (as the reference does; reset() returns to rest).  hard: integers 0 / 1; soft: levels 0 and 2^quant_level - 1,
        int() of every value; unquant: levels 0.0 and 1.0 in float64."""
        x = self._received(x, metric_type, quant_level, 1)
        metric = _METRICS[metric_type]
        return self._kernel().decode(x, metric, quant_level).astype(np.float64)

    def viterbi_decoder_rows(self, x2d, metric_type='soft', quant_level=3):
        """Beyond the reference: every row of x2d an independent frame decoded from rest, all in one launch; (nrow, nsym - Depth + 1)
        float64.  Neither reads nor changes the state viterbi_decoder carries."""
        x = self._received(x2d, metric_type, quant_level, 2)
        if x.shape[0] == 0:
            return np.zeros((0, max(0, -(-x.shape[1] // self.rate.denominator) - self.decision_depth + 1)))
        metric = _METRICS[metric_type]
        return self._kernel().decode_rows(x, metric, quant_level).astype(np.float64)

    # ------------------------------------------------------------------ host restatement
    def viterbi_decoder_host(self, x, metric_type='soft', quant_level=3, carry=True):
        """The reference's decoder in float64 NumPy, vectorised over the states (no GPU).  carry=True continues from and updates this
        object's own host-side decoder state, as the reference's calls do; carry=False decodes from rest and leaves it alone."""
        x = self._received(x, metric_type, quant_level, 1)
        if carry:
            cm, hist = self._host_cm[None].copy(), self._host_hist[None].copy()
        else:
            cm, hist = np.zeros((1, self.Nstates)), np.zeros((1,) + self._host_hist.shape, dtype=np.uint64)
        y, cm, hist = self._host_run(x[None], metric_type, quant_level, cm, hist)
        if carry:
            self._host_cm, self._host_hist = cm[0], hist[0]
        return y[0]

    def viterbi_decoder_rows_host(self, x2d, metric_type='soft', quant_level=3):
        """viterbi_decoder_host(row, carry=False) of every row, vectorised over rows and states: the yardstick of viterbi_decoder_rows."""
        x = self._received(x2d, metric_type, quant_level, 2)
        nrow = x.shape[0]
        return self._host_run(x, metric_type, quant_level, np.zeros((nrow, self.Nstates)),
                              np.zeros((nrow,) + self._host_hist.shape, dtype=np.uint64))[0]

    def _host_run(self, x, metric_type, quant_level, cm, hist):
        """x: (nrow, nval) validated values; cm: (nrow, Ns) float64 metrics, hist: (nrow, Ns, words) uint64 histories (newest bit = bit 0)"""
        R, D = self.rate.denominator, self.decision_depth
        nrow, nval = x.shape
        nsym = -(-nval // R)
        # the 2^R possible branch metrics of every symbol, summed in value order like bm_calc
        sym = np.full((nrow, nsym * R), -1.0)
        sym[:, :nval] = x
        sym = sym.reshape(nrow, nsym, 1, R)
        bits = ((np.arange(2 ** R)[:, None] >> (R - 1 - np.arange(R))) & 1).astype(np.float64)     # [word, k]: first value = most significant bit
        if metric_type == 'hard':
            dist = np.where(sym < 0, 0.0, np.abs(sym - bits))    # (a value behind the end of the stream counts nothing)
        elif metric_type == 'soft':
            d = sym - (2 ** int(quant_level) - 1) * bits
            dist = d * d
        else:
            d = sym - bits
            dist = d * d
        BM = dist[..., 0] + dist[..., 1]
        if R == 3:
            BM = BM + dist[..., 2]
        nw = hist.shape[2]
        ow, ob = (D - 1) // 64, np.uint64((D - 1) % 64)
        one, s63 = np.uint64(1), np.uint64(63)
        p0, p1, b1, b2, u = self._p0, self._p1, self._bits1, self._bits2, self._u
        rows = np.arange(nrow)
        y = np.zeros((nrow, max(0, nsym - D + 1)))
        for t in range(nsym):
            bm = BM[:, t]
            d1 = bm[:, b1] + cm[:, p0]
            d2 = bm[:, b2] + cm[:, p1]
            keep = d1 <= d2
            cm = np.where(keep, d1, d2)
            src = np.take_along_axis(hist, np.where(keep, p0, p1)[:, :, None], axis=1)
            hist = src << one
            hist[:, :, 0] |= u
            if nw > 1:
                hist[:, :, 1:] |= src[:, :, :-1] >> s63
            if t >= D - 1:
                y[:, t - (D - 1)] = (hist[rows, np.argmin(cm, axis=1), ow] >> ob) & one
        return y, cm, hist

    # ------------------------------------------------------------------ encoder and puncturing (host, by design)
    def conv_encoder(self, input, state):
        """output, state = conv_encoder(input, state): a GF(2) FIR over the input bits and the K - 1 state bits (newest first)."""
        K, R = self.constraint_length, self.rate.denominator
        if len(state) != K - 1 or set(state) - {'0', '1'}:
            raise ValueError("conv_encoder: the state must be a string of %d binary digits" % (K - 1))
        u = np.asarray(input)
        if u.size == 0:
            return np.zeros(0), state
        if u.ndim != 1 or np.any((u != 0) & (u != 1)):
            raise ValueError("conv_encoder: the input must be a one-dimensional sequence of bits 0 / 1")
        ext = np.concatenate((np.array([int(c) for c in state[::-1]], dtype=np.int64), u.astype(np.int64)))   # oldest first
        n = u.size
        out = np.zeros((n, R), dtype=np.int64)
        for j in range(R):
            for m in range(K):
                if self._taps[j, m]:
                    out[:, j] ^= ext[K - 1 - m:K - 1 - m + n]
        return out.reshape(-1).astype(np.float64), "".join(str(int(v)) for v in ext[::-1][:K - 1])

    def puncture(self, code_bits, puncture_pattern=('110', '101')):
        """The serial rate-1/2 bits [G1 G2 G1 G2 ...] with the positions the pattern marks 0 removed."""
        code_bits = np.asarray(code_bits)
        L_pp = len(puncture_pattern[0])
        n_words = len(code_bits) // 2
        if 2 * n_words != len(code_bits):
            warnings.warn('Number of code bits must be even!')
            warnings.warn('Truncating bits to be compatible.')
        periods = n_words // L_pp
        if L_pp * periods != n_words:
            warnings.warn('Code bit length is not a multiple pp = %d!' % L_pp)
            warnings.warn('Truncating bits to be compatible.')
        c = code_bits[:2 * L_pp * periods].reshape(periods, L_pp, 2)
        keep1 = [k for k, g in enumerate(puncture_pattern[0]) if g == '1']
        keep2 = [k for k, g in enumerate(puncture_pattern[1]) if g == '1']
        return np.stack((c[:, keep1, 0].reshape(-1), c[:, keep2, 1].reshape(-1)), axis=1).reshape(-1)

    def depuncture(self, soft_bits, puncture_pattern=('110', '101'), erase_value=3.5):
        """The punctured soft bits back in their rate-1/2 positions, erase_value where a bit was removed."""
        soft_bits = np.asarray(soft_bits)
        L_pp = len(puncture_pattern[0])
        L_pp1 = sum(1 for g in puncture_pattern[0] if g == '1')
        n_words = len(soft_bits) // 2
        if 2 * n_words != len(soft_bits):
            warnings.warn('Number of soft bits must be even!')
            warnings.warn('Truncating bits to be compatible.')
        periods = n_words // L_pp1
        if L_pp1 * periods != n_words:
            warnings.warn('Number of soft bits per puncture period is %d' % L_pp1)
            warnings.warn('The number of soft bits is not a multiple')
            warnings.warn('Truncating soft bits to be compatible.')
        s = soft_bits[:2 * n_words].reshape(n_words, 2)[:L_pp1 * periods].reshape(periods, L_pp1, 2)
        y = np.full((periods, L_pp, 2), float(erase_value))
        y[:, [k for k, g in enumerate(puncture_pattern[0]) if g == '1'], 0] = s[:, :, 0]
        y[:, [k for k, g in enumerate(puncture_pattern[1]) if g == '1'], 1] = s[:, :, 1]
        return y.reshape(-1)

    # ------------------------------------------------------------------ the same three over the rows of a frame set, on the GPU
    def _encoder(self):
        if self._enc_kern is None:
            self._enc_kern = _ffi.ConvCodeKernel(self.G_polys)
        return self._enc_kern

    def conv_encoder_rows(self, bits2d, state=None):
        """Beyond the reference: code2d, states = conv_encoder_rows(bits2d, state=None).  Row r of code2d (float64, (nrow, R n)) and
        states[r] are conv_encoder(bits2d[r], state_r); state is None (every row from rest), one string for all rows, or a sequence of nrow
        strings.  One launch over (row, run of bits) pairs (csrc/convcode.hip): a 1-row array is the long-stream form."""
        K, R = self.constraint_length, self.rate.denominator
        u = np.asarray(bits2d)
        if u.ndim != 2:
            raise ValueError("conv_encoder_rows takes a 2-D array, one frame per row; conv_encoder encodes one stream")
        nrow, n = u.shape
        if u.size and np.any((u != 0) & (u != 1)):
            raise ValueError("conv_encoder_rows: the input must hold bits 0 / 1")
        if state is None:
            states = ['0' * (K - 1)]
        elif isinstance(state, str):
            states = [state]
        else:
            states = list(state)
            if len(states) != nrow:
                raise ValueError("conv_encoder_rows: one state, or one per row (got %d for %d rows)" % (len(states), nrow))
        for s in states:
            if not isinstance(s, str) or len(s) != K - 1 or set(s) - {'0', '1'}:
                raise ValueError("conv_encoder_rows: a state must be a string of %d binary digits" % (K - 1))
        if nrow == 0 or n == 0:
            return np.zeros((nrow, R * n)), [states[r if len(states) > 1 else 0] for r in range(nrow)]
        code, out = self._encoder().encode_rows(u.astype(np.uint8), np.array([int(s, 2) for s in states], dtype=np.uint8))
        return code.astype(np.float64), [binary(int(v), K - 1) for v in out]

    def puncture_rows(self, code2d, puncture_pattern=('110', '101')):
        """Beyond the reference: row r of the result is puncture(code2d[r], puncture_pattern), in code2d's dtype (elements of 1, 2, 4 or 8
        bytes); the truncation warnings of the 1-D method, once per call.  Patterns of at most 64 digits, equally long, with the same
        number of ones (else ValueError)."""
        x = np.asarray(code2d)
        if x.ndim != 2:
            raise ValueError("puncture_rows takes a 2-D array, one frame per row; puncture takes one stream")
        _ffi.pattern_masks(puncture_pattern)
        L_pp = len(puncture_pattern[0])
        n_words = x.shape[1] // 2
        if 2 * n_words != x.shape[1]:
            warnings.warn('Number of code bits must be even!')
            warnings.warn('Truncating bits to be compatible.')
        if L_pp * (n_words // L_pp) != n_words:
            warnings.warn('Code bit length is not a multiple pp = %d!' % L_pp)
            warnings.warn('Truncating bits to be compatible.')
        return _ffi.puncture_rows(x, puncture_pattern)

    def depuncture_rows(self, soft2d, puncture_pattern=('110', '101'), erase_value=3.5):
        """Beyond the reference: row r of the result (float64) is depuncture(soft2d[r], puncture_pattern, erase_value); the truncation
        warnings of the 1-D method, once per call."""
        x = np.asarray(soft2d)
        if x.ndim != 2:
            raise ValueError("depuncture_rows takes a 2-D array, one frame per row; depuncture takes one stream")
        _ffi.pattern_masks(puncture_pattern)
        L_pp1 = sum(1 for g in puncture_pattern[0] if g == '1')
        n_words = x.shape[1] // 2
        if 2 * n_words != x.shape[1]:
            warnings.warn('Number of soft bits must be even!')
            warnings.warn('Truncating bits to be compatible.')
        if L_pp1 * (n_words // L_pp1) != n_words:
            warnings.warn('Number of soft bits per puncture period is %d' % L_pp1)
            warnings.warn('The number of soft bits is not a multiple')
            warnings.warn('Truncating soft bits to be compatible.')
        return _ffi.depuncture_rows(x.astype(np.float64), puncture_pattern, float(erase_value))

    # ------------------------------------------------------------------ plots: out of scope
    def trellis_plot(self, fsize=(6, 4)):
        """Plotting helper: out of scope here; delegates to an installed sk_dsp_comm."""
        return _delegate_plot(self, "trellis_plot", fsize)

    def traceback_plot(self, fsize=(6, 4)):
        """Plotting helper: out of scope here; delegates to an installed sk_dsp_comm (whose object has decoded nothing: the trellis
        paths of this decoder live on the device and are not mirrored)."""
        return _delegate_plot(self, "traceback_plot", fsize)


def _delegate_plot(obj, method, *args):
    try:
        import sk_dsp_comm.fec_conv as ref
    except Exception:
        raise NotImplementedError("FECConv.%s is a matplotlib helper outside the accelerated path; "
                                  "install scikit-dsp-comm to use it" % method)
    return getattr(ref.FECConv(obj.G_polys, obj.decision_depth), method)(*args)
