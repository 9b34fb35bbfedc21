"""Gray-coded QAM / MPSK baseband transmitters with the signatures of sk_dsp_comm.digitalcom
(SURVEY.md 8f-2).  Symbol mapping is vectorised NumPy on the host; the expensive step,
lfilter(b, 1, upsample(x_IQ, ns)) (digitalcom.py:1676, 1821), is one polyphase interpolation on
the GPU (sigsys.pulse_shape -> multirate_FIR.up -> fir_direct.hip / fir_ols.hip).

  qam_gray_encode_bb(n_symb, ns, mod, pulse, alpha, m_span, ext_data)   digitalcom.py:1584-1681
  mpsk_gray_encode_bb(n_symb, ns, mod, pulse, alpha, m_span, ext_data)  digitalcom.py:1742-1826
  qam_bb, mpsk_bb, gmsk_bb, rz_bits, time_delay (constant delay)         digitalcom.py:418-492, 613-667, 585-610, 998-1048, 1089-1131
  farrow_resample(x, fs_old, fs_new, i_ord, alpha)                       digitalcom.py:53-235
  my_psd(x, NFFT, Fs)                                                    digitalcom.py:1051-1086  (sigsys.my_psd: csrc/psd.hip)
  bit_errors(tx_data, rx_data, n_corr, n_transient)                      digitalcom.py:353-415    (the count: csrc/convcode.hip)
  qam_gray_decode(x_hat, mod), mpsk_gray_decode(x_hat, mod)              digitalcom.py:1684-1739, 1829-1883  (csrc/symmap.hip)
  qam_gray_map_rows, mpsk_gray_map_rows, qam_gray_decode_rows, mpsk_gray_decode_rows: frame sets, one launch (csrc/symmap.hip)
  xcorr(x1, x2, n_lags), qam_sep, qpsk_bep, bpsk_bep                     digitalcom.py:1163-1179, 495-582, 723-790, 793-846  (csrc/symerr.hip)
  qam_sep_rows, qpsk_bep_rows, bpsk_bep_rows: aligned frame sets, no search, one launch of the fused count (csrc/symerr.hip)

farrow_resample, the arbitrary-ratio resampler, is its own engine (csrc/farrow.hip): each output is a 4-tap FIR whose taps
are polynomials in a fractional delay, evaluated on the GPU for all outputs at once (the reference loops over them in Python).
"""
import math
import warnings
from logging import getLogger

import numpy as np

from . import _ffi, config

log = getLogger(__name__)

from .sigsys import upsample, downsample, cic, rc_imp, sqrt_rc_imp, pulse_shape, _pulse, pulse_shape_rows, matched_filter_rows  # noqa: F401  (re-exported like digitalcom.py:40-47)


def _farrow_len(n, Ts_old, Ts_new):
    """len(np.arange(0, Ts_old*(n-3) + Ts_old, Ts_new)) without the arange (what csrc/farrow_core.hpp's out_len computes)."""
    if Ts_new == 0:
        raise ZeroDivisionError("float division by zero")
    q = (Ts_old * (n - 3) + Ts_old) / Ts_new
    if math.isnan(q):
        raise ValueError("arange: cannot compute length")
    if math.isinf(q):
        raise ValueError("Maximum allowed size exceeded")
    return max(0, math.ceil(q))


def farrow_resample(x, fs_old, fs_new, i_ord=3, alpha=1 / 2):
    """Resample x from fs_old to fs_new, any ratio, with a Farrow interpolator of order i_ord (digitalcom.py:53-235).

    Output j sits at t = j / fs_new; with n_old = floor(t fs_old) and mu its fractional part (both float64, rounded as the
    reference rounds them) it is a cubic (i_ord=3), parabolic (i_ord=2, shaped by alpha) or linear (i_ord=1) interpolation
    of x[n_old-2 .. n_old+1] -- one GPU kernel for all outputs (csrc/farrow.hip).  len(y) = len(np.arange(0, (len(x)-2)/fs_old,
    1/fs_new)).  The result is float64 / complex128 like the reference's (float32 / complex64 inputs keep their own width
    with config.strict_dtype = False); float32 / complex64 inputs are interpolated in float32 unless config.precision is
    "double", float64 / complex128 ones always in float64.  Conventions beyond the reference's: integer arrays run as
    float64 (the reference's lfilter rejects them), and x must be one-dimensional (ValueError otherwise)."""
    if i_ord not in (1, 2, 3):
        raise ValueError('Error: I_ord must 1, 2, or 3')
    if np.size(x) == 0:
        raise ValueError("v cannot be empty")   # (what the reference's lfilter -> np.convolve raises)
    Ts_old = 1 / float(fs_old)
    Ts_new = 1 / float(fs_new)
    n_out = _farrow_len(len(x), Ts_old, Ts_new)
    if not hasattr(x, "dtype"):
        raise AttributeError("'%s' object has no attribute 'dtype'" % type(x).__name__)
    if x.ndim != 1:
        raise ValueError("farrow_resample: x must be one-dimensional (got shape %r)" % (x.shape,))
    from .sigsys import _gpu_dtype
    xg = np.ascontiguousarray(_gpu_dtype(x))
    wide = bool(config.strict_dtype)
    out_dt = np.result_type(xg.dtype, np.float64) if wide else xg.dtype
    if n_out == 0:
        return np.zeros(0, dtype=out_dt)
    a = float(alpha) if i_ord == 2 else 0.5
    return _ffi.farrow(xg, Ts_old, Ts_new, int(i_ord), a, wide=wide, f64=config.precision == "double")


def my_psd(x, NFFT=2 ** 10, Fs=1):
    """matplotlib.mlab.psd(x, NFFT, Fs) as two arrays (digitalcom.py:1051-1086): sigsys.my_psd under the reference's
    parameter names.  Returns (Px, f)."""
    from .sigsys import my_psd as _my_psd
    return _my_psd(x, NFFT, Fs)


def _word_values(data, width):
    """MSB-first integer value of consecutive `width`-bit words."""
    w = 2 ** np.arange(width - 1, -1, -1)
    return np.asarray(data).reshape(-1, width) @ w


def _gray_lut(width):
    """The reference's bin2gray tables: entry k is the running XOR of k's bits from the MSB down."""
    k = np.arange(2 ** width)
    v = k.copy()
    shift = 1
    while shift < width:
        v ^= v >> shift
        shift *= 2
    return v


def _take_bits(n_symb, bits_per_symbol, ext_data):
    if n_symb is None:
        n_symb = int(np.floor(len(ext_data) / bits_per_symbol))
        data = np.asarray(ext_data)[:n_symb * bits_per_symbol]
    else:
        data = np.random.randint(0, 2, size=bits_per_symbol * n_symb)
    return n_symb, data


def _shape(x_iq, ns, pulse, alpha, m_span):
    b = _pulse(pulse, ns, alpha, m_span, err='pulse shape must be src, rc, or rect')
    return pulse_shape(x_iq, b, ns), b / sum(b)


def qam_gray_encode_bb(n_symb, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, ext_data=None):
    """Gray-mapped square QAM complex baseband transmitter: (x, b, tx_data)."""
    if mod not in (2, 4, 16, 64, 256):
        raise ValueError('M must be 2, 4, 16, 64, 256')
    bps = int(np.log2(mod))
    n_symb, data = _take_bits(n_symb, bps, ext_data)
    x_m = np.sqrt(mod) - 1
    if mod == 2:  # BPSK special case
        x_iq = 2 * data - 1
        x_m = 1
    else:
        half = bps // 2
        words = _word_values(data, half).reshape(n_symb, 2)  # [I word, Q word] per symbol, MSB first
        lut = _gray_lut(half)
        x_iq = (2 * lut[words[:, 0]] - x_m) + 1j * (2 * lut[words[:, 1]] - x_m)
    if ns > 1:
        x, b = _shape(x_iq, ns, pulse, alpha, m_span)
        return x / x_m, b, data
    return x_iq / x_m, 1, data


def mpsk_gray_encode_bb(n_symb, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, ext_data=None):
    """Gray-mapped M-PSK complex baseband transmitter: (x, b, tx_data)."""
    if mod not in (2, 4, 8, 16, 32):
        raise ValueError('M must be 2, 4, 8, 16, or 32')
    bps = int(np.log2(mod))
    n_symb, data = _take_bits(n_symb, bps, ext_data)
    if mod == 2:
        x_iq = 2 * data - 1
    else:
        idx = _gray_lut(bps)[_word_values(data, bps)]
        phase = 2 * np.pi * idx / mod + (np.pi / mod if mod == 4 else 0.0)
        x_iq = np.exp(1j * phase)
    if ns > 1:
        x, b = _shape(x_iq, ns, pulse, alpha, m_span)
        return x, b, data
    return x_iq, 1, data


# ---- Gray demapping and the symbol mapping over frame sets (csrc/symmap.hip) -----------------------------------------
def _sym_input(x_hat, name):
    """x_hat as the kernels take it: one-dimensional complex64 / complex128.  Real input is widened to complex, integers run as float64,
    float32 / complex64 stay and are widened exactly on the device."""
    x = np.asarray(x_hat)
    if x.ndim != 1:
        raise ValueError("%s: x_hat must be one-dimensional (got shape %r)" % (name, x.shape))
    if x.dtype.kind in "biu":
        x = x.astype(np.float64)
    if x.dtype.kind not in "fc":
        raise TypeError("%s: x_hat must be numeric (got %s)" % (name, x.dtype))
    if x.dtype == np.complex64 or x.dtype == np.float32 or x.dtype == np.float16:
        return np.ascontiguousarray(x, dtype=np.complex64)
    return np.ascontiguousarray(x, dtype=np.complex128)


def _qam_words_host(x, mod, r):
    """the reference's decision for complex128 symbols x and r = 1.0 / s: (kI, kQ) int16"""
    x_m = 1 if mod == 2 else np.sqrt(mod) - 1
    x = np.asarray(x, dtype=np.complex128)
    with np.errstate(over="ignore"):
        kr, ki = (x.real * r + x_m) / 2, (x.imag * r + x_m) / 2           # (x / s is x * (1.0 / s) in NumPy: complex array by real scalar)
    return np.int16(np.clip(np.rint(kr), 0, x_m)), np.int16(np.clip(np.rint(ki), 0, x_m))


def _bits_of_words(words, width):
    """MSB-first bits of each word: (n, width) uint8"""
    return ((np.asarray(words, dtype=np.int64)[:, None] >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8)


def _qam_bits_host(x, mod, r):
    bps = _ffi.sym_bits(_ffi.QAM, mod)
    kI, kQ = _qam_words_host(x, mod, r)
    if mod == 2:
        return kI.astype(np.uint8)
    half = bps // 2
    return np.hstack((_bits_of_words(kI ^ (kI >> 1), half), _bits_of_words(kQ ^ (kQ >> 1), half))).reshape(-1)


def _qam_scale_host(x, mod):
    """r = 1.0 / (np.std(x) * sqrt(3 / (2 (mod - 1)))) of complex128 symbols; ValueError where it is zero or not finite"""
    with np.errstate(all="ignore"):
        s = np.std(np.asarray(x, dtype=np.complex128)) * np.sqrt(3 / (2 * (mod - 1)))
        r = 1.0 / s if s != 0 else np.inf
    return _check_scale(np.array([r]))[0]


def _check_scale(r):
    if not np.all(np.isfinite(r)) or np.any(r == 0):
        raise ValueError("qam_gray_decode: the scale np.std(x_hat) is zero or not finite (an all-equal frame or a non-finite sample)")
    return r


def _mpsk_bits_host(x, mod):
    bps = _ffi.sym_bits(_ffi.MPSK, mod)
    x = np.asarray(x, dtype=np.complex128)
    if mod == 4:
        x = x * np.exp(-1j * np.pi / 4)
    idx = np.mod(np.rint(np.angle(x) * mod / 2 / np.pi).astype(np.int64), mod)
    return _bits_of_words(idx ^ (idx >> 1), bps).reshape(-1)


def qam_gray_decode_host(x_hat, mod=4):
    """qam_gray_decode in vectorised NumPy (no GPU): the yardstick of qam_gray_decode.  The symbols are widened to complex128 first, then the
    reference's four steps."""
    _ffi.sym_bits(_ffi.QAM, mod)
    x = _sym_input(x_hat, "qam_gray_decode").astype(np.complex128)
    if x.size == 0:
        return np.zeros(0, dtype=np.int64)
    bits = _qam_bits_host(x, mod, _qam_scale_host(x, mod))
    return bits.astype(np.int16 if mod == 2 else np.int64)


def mpsk_gray_decode_host(x_hat, mod=4):
    """mpsk_gray_decode in vectorised NumPy (no GPU): the yardstick of mpsk_gray_decode."""
    _ffi.sym_bits(_ffi.MPSK, mod)
    x = _sym_input(x_hat, "mpsk_gray_decode").astype(np.complex128)
    if x.size == 0:
        return np.zeros(0, dtype=np.int64)
    return _mpsk_bits_host(x, mod).astype(np.int64)


def _sym_rows_input(x2d, name):
    x = np.asarray(x2d)
    if x.ndim != 2:
        raise ValueError("%s: a 2-D array, one frame per row" % name)
    return _sym_input(x.reshape(-1), name).reshape(x.shape)


def qam_gray_decode_rows(x2d, mod=4, start=0, step=1):
    """Beyond the reference: every row of x2d is its own frame with its own np.std; symbol k of a row is x2d[row, start + k * step] (the
    idiom z[start::ns] behind the matched filter, without a compacting pass).  Returns uint8 (rows, n_symb * bps).  Two launches for the
    rows' scales, one for the decisions (csrc/symmap.hip).  A row whose scale is zero or not finite raises ValueError."""
    _ffi.sym_bits(_ffi.QAM, mod)
    x = _sym_rows_input(x2d, "qam_gray_decode_rows")
    n = _ffi.sym_count(x.shape[1], start, step)
    if x.shape[0] == 0 or n == 0:
        return np.zeros((x.shape[0], 0), dtype=np.uint8)
    r = _check_scale(_ffi.qam_scale_rows(x, mod, start, step))
    return _ffi.gray_demap_rows(x, _ffi.QAM, mod, start, step, r)


def mpsk_gray_decode_rows(x2d, mod=4, start=0, step=1):
    """Beyond the reference: mpsk_gray_decode of every row's x2d[row, start::step] in one launch; uint8 (rows, n_symb * bps)."""
    _ffi.sym_bits(_ffi.MPSK, mod)
    x = _sym_rows_input(x2d, "mpsk_gray_decode_rows")
    n = _ffi.sym_count(x.shape[1], start, step)
    if x.shape[0] == 0 or n == 0:
        return np.zeros((x.shape[0], 0), dtype=np.uint8)
    return _ffi.gray_demap_rows(x, _ffi.MPSK, mod, start, step)


def qam_gray_decode(x_hat, mod=4):
    """data_hat = qam_gray_decode(x_hat, mod=4), digitalcom.py:1684-1739: x_hat / (np.std(x_hat) * sqrt(3 / (2 (mod - 1)))), each component
    decided to the nearest of sqrt(mod) levels, Gray decoded to [I bits, Q bits] per symbol, MSB first.  The reference loops over the symbols
    in Python; here np.std is a deterministic float64 merge of partial moments on the GPU and every decision is the reference's own float64
    operations in its order (csrc/symmap.hip).  Returns int64 (mod 2: the int16 level array, like the reference).

    Deliberate differences (tests/golden/g22_conventions.json): a bad order raises the reference's ValueError for an empty x_hat too;
    an empty x_hat returns an empty int64 array without the reference's warnings; a scale that is zero or not finite (an all-equal frame, a
    non-finite sample) raises ValueError where the reference casts NaN to an integer; real input is widened to complex (the reference then
    divides instead of multiplying by the reciprocal: one ulp, on a threshold only); integer input runs as float64; float32 / complex64
    input is widened exactly and decided in float64 (the reference takes np.std in float32)."""
    _ffi.sym_bits(_ffi.QAM, mod)
    x = _sym_input(x_hat, "qam_gray_decode")
    if x.size == 0:
        return np.zeros(0, dtype=np.int64)
    bits = qam_gray_decode_rows(x.reshape(1, -1), mod)[0]
    return bits.astype(np.int16 if mod == 2 else np.int64)


def mpsk_gray_decode(x_hat, mod=4):
    """data_hat = mpsk_gray_decode(x_hat, mod=4), digitalcom.py:1829-1883: np.mod(rint(angle(x_hat) * mod / 2 / pi), mod) (mod 4: of x_hat
    rotated by exp(-1j pi / 4)), Gray decoded, MSB first, int64.  The reference's quirks are kept: mod 2 decodes -1 to bit 1, 0 decodes as
    angle 0, -1 - 0j as angle -pi.  One launch (csrc/symmap.hip).  Deliberate differences: as qam_gray_decode (bad order, empty input,
    real / integer / single-precision input: the angle is always taken in float64)."""
    _ffi.sym_bits(_ffi.MPSK, mod)
    x = _sym_input(x_hat, "mpsk_gray_decode")
    if x.size == 0:
        return np.zeros(0, dtype=np.int64)
    return mpsk_gray_decode_rows(x.reshape(1, -1), mod)[0].astype(np.int64)


def _map_rows(kind, bits2d, mod, dtype, name):
    _ffi.sym_bits(kind, mod)
    bits = np.asarray(bits2d)
    if bits.ndim != 2:
        raise ValueError("%s: a 2-D array of bits, one frame per row" % name)
    if bits.size and np.any((bits != 0) & (bits != 1)):
        raise ValueError("%s: bits 0 / 1 only" % name)
    if np.dtype(dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise TypeError("%s: dtype must be complex64 or complex128" % name)
    return _ffi.gray_map_rows(bits.astype(np.uint8), kind, mod, np.dtype(dtype))


def qam_gray_map_rows(bits2d, mod=4, dtype=np.complex128):
    """Beyond the reference: the symbol sequence qam_gray_encode_bb builds before shaping (x_IQ / x_m), for every row of bits at once on the
    GPU; always complex (mod 2: imaginary part 0).  Trailing bits that do not fill a symbol are dropped, as the reference truncates ext_data.
    complex128 values are bit-identical to the reference's, complex64 ones their float32 roundings (a table lookup of host-computed points)."""
    return _map_rows(_ffi.QAM, bits2d, mod, dtype, "qam_gray_map_rows")


def mpsk_gray_map_rows(bits2d, mod=4, dtype=np.complex128):
    """Beyond the reference: the symbol sequence mpsk_gray_encode_bb builds before shaping (x_IQ), as qam_gray_map_rows."""
    return _map_rows(_ffi.MPSK, bits2d, mod, dtype, "mpsk_gray_map_rows")


# ---- the Gray transmitters over frame sets: mapping and pulse shaping on the device (csrc/symmap.hip, csrc/pulse.hip) ----
def _encode_rows_args(kind, bits2d, ns, mod, pulse, alpha, m_span, dtype, name):
    """(bits uint8 (nrow, n bps), n, taps, returned b): the checks of the 1-D transmitters in their order and with their messages"""
    bps = _ffi.sym_bits(kind, mod)
    bits = np.asarray(bits2d)
    if bits.ndim != 2:
        raise ValueError("%s: a 2-D array of bits, one frame per row" % name)
    if bits.size and np.any((bits != 0) & (bits != 1)):
        raise ValueError("%s: bits 0 / 1 only" % name)
    if np.dtype(dtype) not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise TypeError("%s: dtype must be complex64 or complex128" % name)
    if int(ns) != ns or ns < 1:
        raise ValueError("%s: ns must be a positive integer" % name)
    n = bits.shape[1] // bps
    bits = np.ascontiguousarray(bits[:, :n * bps], dtype=np.uint8)
    if ns > 1:
        taps = _pulse(pulse, int(ns), alpha, m_span, err='pulse shape must be src, rc, or rect')
        return bits, n, np.ascontiguousarray(taps, dtype=np.float64), taps / sum(taps)
    return bits, n, np.ones(1), 1


def _encode_rows(kind, bits2d, ns, mod, pulse, alpha, m_span, dtype, name, host):
    bits, n, taps, b = _encode_rows_args(kind, bits2d, ns, mod, pulse, alpha, m_span, dtype, name)
    ns, dtype, nrow = int(ns), np.dtype(dtype), bits.shape[0]
    table, scale = _ffi.gray_levels(kind, mod, dtype)
    if host or not _ffi.pulse_served(taps.size, ns):
        sym = _ffi.gray_map_rows_host(bits, kind, mod, dtype, table=table)
        return (_ffi.pulse_shape_rows_host if host else pulse_shape_rows)(sym, taps, ns, scale), b
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n * ns), dtype=dtype), b
    bd, sd, yd = _ffi.device_bytes_of(bits), _ffi.DeviceArray(nrow * n, dtype), _ffi.DeviceArray(nrow * n * ns, dtype)
    try:   # bits -> points -> waveform, nothing on the host in between
        _ffi.gray_map_rows_dev(bd.ptr, bits.shape[1], n, nrow, kind, mod, dtype, sd.ptr, table=table)
        _ffi.PulseKernel(taps, dtype).shape_rows_dev(sd, yd, n, nrow, ns, scale)
        return yd.to_host().reshape(nrow, n * ns), b
    finally:
        for d in (bd, sd, yd):
            d.free()


def qam_gray_encode_bb_rows(bits2d, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, dtype=np.complex128):
    """Beyond the reference: qam_gray_encode_bb(None, ns, mod, pulse, alpha, m_span, ext_data=row) for every row of bits2d at once, on the device:
    the Gray mapping kernel (the integer levels 2 lut - x_m), then the shaping kernel with the factor 1 / x_m behind its sum, with no host data in
    between.  Returns (x2d, b): x2d (nrow, n_symb ns) of `dtype`, always complex (mod 2: imaginary part 0); b the reference's unity-gain
    b / sum(b), or 1 for ns == 1.  Trailing bits that do not fill a symbol are dropped.  Each row lies within the summation-order bound of the
    reference and equals qam_gray_encode_bb_rows_host bit for bit."""
    return _encode_rows(_ffi.QAM, bits2d, ns, mod, pulse, alpha, m_span, dtype, "qam_gray_encode_bb_rows", False)


def qam_gray_encode_bb_rows_host(bits2d, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, dtype=np.complex128):
    """qam_gray_encode_bb_rows in NumPy (no GPU): gray_map_rows_host on the same levels, then pulse_shape_rows_host with the same factor."""
    return _encode_rows(_ffi.QAM, bits2d, ns, mod, pulse, alpha, m_span, dtype, "qam_gray_encode_bb_rows", True)


def mpsk_gray_encode_bb_rows(bits2d, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, dtype=np.complex128):
    """Beyond the reference: mpsk_gray_encode_bb(None, ns, mod, pulse, alpha, m_span, ext_data=row) for every row of bits2d at once, as
    qam_gray_encode_bb_rows (there is no scale: the points lie on the unit circle)."""
    return _encode_rows(_ffi.MPSK, bits2d, ns, mod, pulse, alpha, m_span, dtype, "mpsk_gray_encode_bb_rows", False)


def mpsk_gray_encode_bb_rows_host(bits2d, ns, mod=4, pulse='rect', alpha=0.35, m_span=6, dtype=np.complex128):
    """mpsk_gray_encode_bb_rows in NumPy (no GPU)."""
    return _encode_rows(_ffi.MPSK, bits2d, ns, mod, pulse, alpha, m_span, dtype, "mpsk_gray_encode_bb_rows", True)


# ---- the remaining lfilter(b, 1, .) callers of digitalcom.py (488, 608, 666, 1047, 1130) ------------------------------
def qam_bb(n_symb, ns, mod='16qam', pulse='rect', alpha=0.35):
    """Square-QAM complex baseband transmitter without Gray mapping (digitalcom.py:418-492): (x, b, tx_data).  The
    random symbols are drawn exactly as the reference draws them (I levels, then Q levels)."""
    b = _pulse(pulse, ns, alpha, 6, err='pulse shape must be src, rc, or rect')
    levels = {'qpsk': 2, '16qam': 4, '64qam': 8, '256qam': 16}.get(mod.lower())
    if levels is None:
        raise ValueError('Unknown mod_type')
    x_i = 2 * np.random.randint(0, levels, n_symb) - (levels - 1)
    x_q = 2 * np.random.randint(0, levels, n_symb) - (levels - 1)
    symb = (x_i + 1j * x_q).astype(np.complex128)
    if levels > 2:
        symb = symb / (levels - 1)
    x = pulse_shape(symb, b, ns) if n_symb else np.zeros(0, dtype=np.complex128)
    return x, b / sum(b), x_i + 1j * x_q


def mpsk_bb(n_symb, ns, mod, pulse='rect', alpha=0.25, m=6):
    """M-ary PSK complex baseband transmitter (digitalcom.py:613-667): (x, b / ns, data)."""
    data = np.random.randint(0, mod, n_symb)
    xs = np.exp(1j * 2 * np.pi / mod * data)
    b = _pulse(pulse, ns, alpha, m, err='pulse type must be rec, rc, or src')
    x = pulse_shape(xs, b, ns) if n_symb else np.zeros(0, dtype=np.complex128)
    if mod == 4:
        x = x * np.exp(1j * np.pi / 4)
    return x, b / float(ns), data


def rz_bits(n_bits, ns, pulse='rect', alpha=0.25, m=6):
    """Return-to-zero 0/1 waveform from random bits (digitalcom.py:998-1048): (x, b / ns, data)."""
    data = np.random.randint(0, 2, n_bits)
    try:
        b = _pulse(pulse, ns, alpha, m, err='pulse type must be rec, rc, or src')
    except ValueError as e:
        # the reference only warns here (digitalcom.py:1045-1046) and then fails on its unassigned `b` (:1047)
        import warnings
        warnings.warn(str(e))
        raise UnboundLocalError("local variable 'b' referenced before assignment")
    x = pulse_shape(data, b, ns) if n_bits else np.zeros(0)
    return x, b / float(ns), data


def gmsk_bb(n_bits, ns, msk=0, bt=0.35):
    """MSK / GMSK complex baseband transmitter (digitalcom.py:585-610): (y, data).  The NRZ shaping and the Gaussian
    pre-modulation filter (8 ns + 1 taps) run on the GPU; the phase accumulation is a host cumsum as in the reference."""
    from .sigsys import nrz_bits
    from . import multirate_helper as mrh
    x, b, data = nrz_bits(n_bits, ns)
    span = 4
    n = np.arange(-span * ns, span * ns + 1)
    p = np.exp(-2 * np.pi ** 2 * bt ** 2 / np.log(2) * (n / float(ns)) ** 2)
    p = p / np.sum(p)
    if msk != 0:
        x = mrh.multirate_FIR(p).filter(x)
    y = np.exp(1j * np.pi / 2 * np.cumsum(x) / ns)
    return y, data


def time_delay(x, d, n=4):
    """Farrow-structure time delay (digitalcom.py:1089-1160).  A Python float / int d is the reference's constant-delay
    branch (:1110-1131): cubic Lagrange taps behind fix(d) whole samples, ONE lfilter call -- filtered on the GPU.
    Anything else is the time-varying branch (:1132-1160, d[k] per sample): a 4-tap gather with polynomial weights,
    y[k] = ((v3 mu + v2) mu + v1) mu + v0,  v_j = W_j . x[k-Nd_k+1 .. k-Nd_k-2],  mu = 1 - frac(d[k]),
    evaluated for all k at once on the host (the reference loops over k in Python; there is no filter call to
    accelerate: every output has its own taps)."""
    from . import multirate_helper as mrh
    if type(d) == float or type(d) == int:   # (the reference's own test, :1110)
        if int(np.fix(d)) < 1 or int(np.fix(d)) > n - 2:
            raise ValueError("time_delay: the integer part of d must lie in [1, n - 2]")
        frac = d - np.fix(d)
        nd = int(np.fix(d))
        b = np.zeros(nd + 4)
        b[nd] = -(frac - 1) * (frac - 2) * (frac - 3) / 6.
        b[nd + 1] = frac * (frac - 2) * (frac - 3) / 2.
        b[nd + 2] = -frac * (frac - 1) * (frac - 3) / 2.
        b[nd + 3] = frac * (frac - 1) * (frac - 2) / 6.
        return mrh.multirate_FIR(b).filter(np.asarray(x))
    x = np.asarray(x)
    d = np.asarray(d, dtype=np.float64)
    if d.ndim == 0:                           # a NumPy scalar: the reference would index it and fail; treat it as constant per sample
        d = np.full(len(x), float(d))
    if len(d) < len(x):
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (len(d), len(d)))   # what d[k] raises in the reference
    d = d[:len(x)]
    if len(x) and (np.fix(np.min(d)) < 1 or np.fix(np.max(d)) > n - 2):
        raise ValueError("time_delay: the integer part of d must lie in [1, n - 2]")
    nd = np.fix(d).astype(np.int64)
    mu = 1.0 - (d - np.fix(d))
    k = np.arange(len(x))
    xr = np.real(x).astype(np.float64) if np.iscomplexobj(x) else x.astype(np.float64)   # y = np.zeros(len(x)): real (:1139)
    taps = np.zeros((4, len(x)))
    for i in range(4):                        # X[Nd-1+i] = x[k - (Nd-1) - i], zero before the start
        idx = k - (nd - 1) - i
        ok = idx >= 0
        taps[i, ok] = xr[idx[ok]]
    w3 = np.array([1. / 6, -1. / 2, 1. / 2, -1. / 6])
    w2 = np.array([0, 1. / 2, -1., 1. / 2])
    w1 = np.array([-1. / 6, 1., -1. / 2, -1. / 3])
    w0 = np.array([0, 0, 1., 0])
    v3, v2, v1, v0 = w3 @ taps, w2 @ taps, w1 @ taps, w0 @ taps
    return ((v3 * mu + v2) * mu + v1) * mu + v0


# ------------------------------------------------------------------------------------------------ bit_errors (digitalcom.py:353-415)
MAX_N_CORR = 65536


def _bits_1d(x, name):
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("bit_errors: %s must be a one-dimensional sequence of bits" % name)
    if x.size and np.any((x != 0) & (x != 1)):
        raise ValueError("bit_errors: %s must hold bits 0 / 1 only" % name)
    return x.astype(np.uint8)


def _check_n_corr(n_corr, n_transient):
    if int(n_corr) != n_corr or n_corr < 1:
        raise ValueError("bit_errors: n_corr must be a positive integer (got %r)" % (n_corr,))
    if n_corr % 2:
        warnings.warn("n_corr needs to be even")
        raise ValueError("bit_errors: n_corr must be even (got %d): the reference centres lag 0 at n_corr / 2" % n_corr)
    if n_corr > MAX_N_CORR:
        raise ValueError("bit_errors: n_corr of at most %d is served (got %d)" % (MAX_N_CORR, n_corr))
    if int(n_transient) != n_transient or n_transient < 0:
        raise ValueError("bit_errors: n_transient must be a non-negative integer (got %r)" % (n_transient,))
    return int(n_corr), int(n_transient)


def bit_errors_search(tx_head, rx_head, n_corr):
    """(kmax, taumax) of the reference's lag and sign search over the first n_corr bits of each stream (bits 0 / 1, zero-padded as +-1
    sequences if shorter), in exact integer arithmetic: the circular correlation of two +-1 / 0 sequences of n_corr <= 65536 values is an
    integer of magnitude <= n_corr, a float64 FFT gets it to within 1e-9, and rounding to the nearest integer restores it.  R1 = -R0;
    phase 0 unless phase 1's maximum is STRICTLY larger; the first index attaining the maximum; lag 0 sits at n_corr / 2 after fftshift.
    Where the exact maximum is attained more than once the reference's pick depends on its FFT's rounding noise; this picks by that order."""
    a, b = np.zeros(n_corr), np.zeros(n_corr)
    t, r = np.asarray(tx_head[:n_corr], dtype=np.int64), np.asarray(rx_head[:n_corr], dtype=np.int64)
    a[:t.size], b[:r.size] = 2 * t - 1, 2 * r - 1
    R0 = np.fft.fftshift(np.rint(np.fft.ifft(np.fft.fft(b) * np.conj(np.fft.fft(a))).real).astype(np.int64))
    R1 = -R0
    kmax = 1 if R1.max() > R0.max() else 0
    R = R1 if kmax else R0
    return kmax, int(np.argmax(R)) - n_corr // 2


def _overlap(n_tx, n_rx, taumax):
    """(tx start, rx start, Bit_count) of the reference's trimming (digitalcom.py:402-411), lengths after the transient"""
    if taumax < 0:
        t0, r0 = min(-taumax, n_tx), 0
    else:
        t0, r0 = 0, min(taumax, n_rx)
    return t0, r0, min(n_tx - t0, n_rx - r0)


def bit_errors_host(tx_data, rx_data, n_corr=1024, n_transient=0):
    """bit_errors in NumPy (no GPU): the yardstick of bit_errors."""
    n_corr, n_transient = _check_n_corr(n_corr, n_transient)
    tx, rx = _bits_1d(tx_data, "tx_data")[n_transient:], _bits_1d(rx_data, "rx_data")[n_transient:]
    if tx.size == 0 or rx.size == 0:
        raise ValueError("bit_errors: no bits behind the transient")
    kmax, taumax = bit_errors_search(tx, rx, n_corr)
    log.info('kmax =  %d, taumax = %d' % (kmax, taumax))
    t0, r0, count = _overlap(tx.size, rx.size, taumax)
    return count, np.sum((tx[t0:t0 + count] ^ rx[r0:r0 + count] ^ kmax).astype(np.int64))


def bit_errors(tx_data, rx_data, n_corr=1024, n_transient=0):
    """(Bit_count, Bit_errors) = bit_errors(tx_data, rx_data, n_corr=1024, n_transient=0), digitalcom.py:353-415: the delay between the two
    0 / 1 streams and a sign inversion of rx are found from the first n_corr bits behind the transient (bit_errors_search: on the host, exact
    integers), then the differing bits are counted over the whole overlap on the GPU (csrc/convcode.hip: bitcount_kernel, the lag as the two
    start offsets, the sign as `invert`).  Returns (int, numpy.int64) like the reference.

    tx_data / rx_data: sequences of bits, or _ffi.DeviceBytes (one byte per bit, all nbytes of it): then only the 2 n_corr bytes of the
    search and the 8 bytes of the count cross to the host.

    Deliberate differences (tests/golden/g21_conventions.json): values other than 0 / 1, an odd n_corr (after the reference's warning) and
    n_corr > 65536 raise ValueError; a tie of the exact correlation maximum is broken by the order above, not by rounding noise."""
    n_corr, n_transient = _check_n_corr(n_corr, n_transient)
    streams = (tx_data,) if tx_data is rx_data else (tx_data, rx_data)      # tx is rx: one stream, one copy
    dev = [isinstance(v, _ffi.DeviceBytes) for v in streams]
    host, heads, lens = [], [], []
    for v, on_dev, name in zip(streams, dev, ("tx_data", "rx_data")):      # every argument check before the device is touched
        if on_dev:
            host.append(None)
            lens.append(v.nbytes - n_transient)
        else:
            host.append(_bits_1d(v, name)[n_transient:])
            lens.append(host[-1].size)
    if min(lens) <= 0:
        raise ValueError("bit_errors: no bits behind the transient")
    bufs = []
    for v, bits, n, name in zip(streams, host, lens, ("tx_data", "rx_data")):
        if bits is None:
            heads.append(v.read(n_transient, min(n, n_corr)))
            if np.any(heads[-1] > 1):
                raise ValueError("bit_errors: %s must hold bits 0 / 1 only" % name)
            bufs.append((v, n_transient))
        else:
            heads.append(bits[:n_corr])
            d = _ffi.DeviceBytes(n)
            d.write(bits)
            bufs.append((d, 0))
    if len(streams) == 1:
        bufs, heads, lens = bufs * 2, heads * 2, lens * 2
    kmax, taumax = bit_errors_search(heads[0], heads[1], n_corr)
    log.info('kmax =  %d, taumax = %d' % (kmax, taumax))
    t0, r0, count = _overlap(lens[0], lens[1], taumax)
    cnt = _ffi.DeviceBytes(8)
    _ffi.bit_count_rows_dev(bufs[0][0].ptr + bufs[0][1] + t0, 0, bufs[1][0].ptr + bufs[1][1] + r0, 0, count, 1, kmax, cnt.ptr)
    errors = cnt.read().view(np.int64)[0]
    cnt.free()
    for (d, _), bits in zip(bufs[:len(streams)], host):
        if bits is not None:
            d.free()
    return count, errors


def bit_errors_rows(tx2d, rx2d):
    """Beyond the reference: (bits_per_row, errors int64[nrow]) over the first min(width) columns of every row, no lag search -- row r of
    FECConv.viterbi_decoder_rows is aligned with tx[r, :nsym - Depth + 1] by construction.  One launch of the count kernel."""
    tx, rx = np.asarray(tx2d), np.asarray(rx2d)
    if tx.ndim != 2 or rx.ndim != 2 or tx.shape[0] != rx.shape[0]:
        raise ValueError("bit_errors_rows: two 2-D arrays with the same number of rows")
    for v in (tx, rx):
        if v.size and np.any((v != 0) & (v != 1)):
            raise ValueError("bit_errors_rows: bits 0 / 1 only")
    n = min(tx.shape[1], rx.shape[1])
    return n, _ffi.bit_count_rows(tx.astype(np.uint8), rx.astype(np.uint8), False, n)


# ------------------------------------------------------------------------------------------------ awgn_channel (digitalcom.py:1259-1281)
def _channel_bits(x, name, ndim):
    x = np.asarray(x)
    if x.ndim != ndim:
        raise ValueError("%s: a %d-D array of bits" % (name, ndim))
    if x.size and np.any((x != 0) & (x != 1)):
        raise ValueError("%s: bits 0 / 1 only" % name)
    return np.ascontiguousarray(x, dtype=np.uint8)


def _channel_sigma(eb_n0_dB):
    var_noise = 10 ** (-eb_n0_dB / 10) / 2
    return float(np.sqrt(var_noise))


def _decisions_as_float(d):
    """the kernel's bytes as the reference's values: (sign + 1) / 2 is 1., 0., 0.5 for an exact zero and nan for what is not a number"""
    return np.array([0.0, 1.0, 0.5, np.nan])[d]


def awgn_channel_rows(bits2d, eb_n0_dB, seed=None):
    """Beyond the reference: (nrow, n) bits -> (nrow, n) uint8 hard decisions, row r through the stream of row r, no float stream in between
    (csrc/channel.hip: awgn_bits_kernel).  A byte is 1 or 0 (2: the sum was exactly zero, 3: it was not a number)."""
    bits = _channel_bits(bits2d, "awgn_channel_rows", 2)
    nrow, n = bits.shape
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n), dtype=np.uint8)
    seed = _ffi.new_seed() if seed is None else seed
    xd = _ffi.device_bytes_of(bits)
    try:
        _ffi.awgn_bits_rows_dev(xd, xd, n, nrow, seed, sigma=_channel_sigma(eb_n0_dB))     # in place
        return xd.read().reshape(nrow, n)
    finally:
        xd.free()


def awgn_channel(x_bits, eb_n0_dB, seed=None):
    """y_bits = awgn_channel(x_bits, eb_n0_dB), digitalcom.py:1259-1281: 0 / 1 -> -1 / +1, noise of variance 10^(-eb_n0_dB / 10) / 2, hard
    decisions back to 0. / 1. (float64, 0.5 for a sum of exactly zero), on the GPU.

    Deliberate differences (tests/golden/g23_conventions.json): the normals are this library's counter-based stream of `seed` (None: 64 bits
    of NumPy's global generator); x_bits is one-dimensional and holds 0 / 1 only (ValueError otherwise); an empty input gives an empty array."""
    bits = _channel_bits(x_bits, "awgn_channel", 1)
    return _decisions_as_float(awgn_channel_rows(bits[None, :], eb_n0_dB, seed)[0])


def awgn_channel_host(x_bits, eb_n0_dB, seed=None):
    """awgn_channel in NumPy (no GPU): the yardstick of awgn_channel."""
    bits = _channel_bits(x_bits, "awgn_channel", 1)
    if bits.size == 0:
        return np.zeros(0)
    seed = _ffi.new_seed() if seed is None else seed
    return _decisions_as_float(_ffi.awgn_bits_rows_host(bits[None, :], _channel_sigma(eb_n0_dB), seed)[0])


# ------------------------------------------------------------------------------------------------ OFDM (digitalcom.py:1284-1547)
# What the reference computes, its quirks included, and the deliberate differences: tests/golden/g24_conventions.json, DESIGN.md 4.19.
def _ofdm_check(name, nf, nc, npb, ncp, rx=False, ht=None):
    nf, nc, npb, ncp = int(nf), int(nc), int(npb), int(ncp)
    if nf < 2 or nf % 2 or nf > nc - 2:
        raise ValueError("%s: nf must be even and 2 <= nf <= nc - 2 (nf = %d, nc = %d)" % (name, nf, nc))
    if npb == 1:
        raise ValueError("%s: npb = 1 leaves no data symbols (the reference divides by zero)" % name)
    if npb < (-1 if rx else 0):
        raise ValueError("%s: npb must be %s0 or at least 2 (npb = %d)" % (name, "-1, " if rx else "", npb))
    if ncp < 0 or ncp > nc:
        raise ValueError("%s: need 0 <= ncp <= nc (ncp = %d, nc = %d)" % (name, ncp, nc))
    if rx and npb == -1 and ht is None:
        raise ValueError("%s: npb = -1 equalises with the known channel: pass ht" % name)
    return nf, nc, npb, ncp


def _ofdm_on_gpu(nc):
    return 64 <= nc <= 4096 and nc & (nc - 1) == 0


def _ofdm_input(x, name, ndim):
    """complex64 / float32 stay single precision (computed in float64, rounded once); everything else is complex128"""
    x = np.asarray(x)
    if x.ndim != ndim:
        raise ValueError("%s: a %d-D array" % (name, ndim))
    single = x.dtype in (np.dtype(np.complex64), np.dtype(np.float32))
    return x.astype(np.complex64 if single else np.complex128, copy=False)


def _ofdm_hht(ht, nf, nc, name):
    """the channel impulse response on the filled carriers: fft(ht, nc) picked by the carrier map"""
    if ht is None:
        return None
    ht = np.asarray(ht)
    if ht.ndim != 1 or ht.size == 0 or ht.size > nc:
        raise ValueError("%s: ht must hold 1 ... nc = %d taps" % (name, nc))
    Ht = np.fft.fft(ht.astype(np.complex128), nc)
    return np.hstack((Ht[1:nf // 2 + 1], Ht[nc - nf // 2:]))


def mux_pilot_blocks(iq_data, npb):
    """IQ_datap = mux_pilot_blocks(iq_data, npb), digitalcom.py:1284-1319, vectorised on the host: a row of ones in front of every npb - 1
    rows of the (N, nf) data.  T = N + N // (npb - 1) + 1 rows, complex128; where npb - 1 divides N the last row is all zeros, not a pilot,
    as in the reference (it assigns into an empty slice there).  npb < 2 raises ValueError (the reference divides by zero at npb = 1)."""
    d = np.asarray(iq_data)
    if d.ndim != 2:
        raise ValueError("mux_pilot_blocks: a 2-D array, one OFDM symbol per row")
    npb = int(npb)
    if npb < 2:
        raise ValueError("mux_pilot_blocks: npb must be at least 2")
    N, nf = d.shape
    out = np.zeros((N + N // (npb - 1) + 1, nf), dtype=np.complex128)
    j = np.arange(out.shape[0])
    pilot = j % npb == 0
    out[pilot] = 1.0
    out[~pilot] = d[j[~pilot] - j[~pilot] // npb - 1]
    if N % (npb - 1) == 0:
        out[-1] = 0.0
    return out


def ofdm_tx_host(iq_data, nf, nc, npb=0, cp=False, ncp=0):
    """ofdm_tx in NumPy (no GPU), float64: the yardstick of the kernel and the path of every nc the kernels do not take."""
    nf, nc, npb, ncp = _ofdm_check("ofdm_tx", nf, nc, npb, ncp)
    x = _ofdm_input(iq_data, "ofdm_tx", 1)
    N = x.size // nf
    s2p = x[:N * nf].reshape(N, nf).astype(np.complex128)
    if npb > 0:
        s2p = mux_pilot_blocks(s2p, npb)
    T, L = s2p.shape[0], nc + (ncp if cp else 0)
    if T == 0:
        return np.zeros(0, dtype=x.dtype)
    buff = np.zeros((T, nc), dtype=np.complex128)
    buff[:, 1:nf // 2 + 1] = s2p[:, :nf // 2]
    buff[:, nc - nf // 2:] = s2p[:, nf // 2:]
    t = np.fft.ifft(buff, axis=1)
    if cp:
        t = np.hstack((t[:, nc - ncp:], t))
    return t.reshape(T * L).astype(x.dtype)


def chan_est_equalize_host(z, npbp, alpha, ht=None):
    """chan_est_equalize in NumPy (no GPU), float64: rows k % npbp == 0 of z are pilots and run H = z[0], H = alpha H + (1 - alpha) z[k];
    the other rows are divided by ht where it is given (the reference), else by the estimate of the latest pilot in front of them."""
    z = _ofdm_input(z, "chan_est_equalize", 2)
    npbp = int(npbp)
    if npbp < 2:
        raise ValueError("chan_est_equalize: npbp must be at least 2")
    N, nf = z.shape
    if ht is not None:
        ht = np.asarray(ht, dtype=np.complex128)
        if ht.shape != (nf,):
            raise ValueError("chan_est_equalize: ht holds the channel on the nf carriers")
    if N == 0:
        return np.zeros((0, nf), dtype=z.dtype), np.full(nf, np.nan + 0j)
    pilots = z[::npbp].astype(np.complex128)
    est = np.empty_like(pilots)
    est[0] = pilots[0]
    for p in range(1, pilots.shape[0]):
        est[p] = alpha * est[p - 1] + (1 - alpha) * pilots[p]
    k = np.arange(N)
    data = k[k % npbp != 0]
    div = ht[None, :] if ht is not None else est[data // npbp]
    with np.errstate(all="ignore"):
        zz = z[data].astype(np.complex128) / div
    return zz.astype(z.dtype), est[-1].copy()


def ofdm_rx_host(x, nf, nc, npb=0, cp=False, ncp=0, alpha=0.95, ht=None):
    """ofdm_rx in NumPy (no GPU), float64: the yardstick of the kernels and the path of every nc they do not take."""
    nf, nc, npb, ncp = _ofdm_check("ofdm_rx", nf, nc, npb, ncp, True, ht)
    x = _ofdm_input(x, "ofdm_rx", 1)
    hht = _ofdm_hht(ht, nf, nc, "ofdm_rx")
    nsym = x.size // (nc + ncp)
    stride, off = (nc + ncp, ncp) if cp else (nc, 0)
    if nsym == 0:
        z = np.zeros((0, nf), dtype=np.complex128)
    else:
        Y = np.fft.fft(x[:nsym * stride].reshape(nsym, stride)[:, off:].astype(np.complex128), axis=1)
        z = np.hstack((Y[:, 1:nf // 2 + 1], Y[:, nc - nf // 2:]))
    if npb > 0:
        z, H = chan_est_equalize_host(z, npb, alpha, hht)
    elif npb == -1:
        H = hht
        with np.errstate(all="ignore"):
            z = z / H[None, :]
    else:
        H = np.ones(nf)
    return z.reshape(-1).astype(x.dtype), H


def ofdm_tx_rows(iq2d, nf, nc, npb=0, cp=False, ncp=0):
    """Beyond the reference: ofdm_tx of every row of a frame set in one launch (csrc/ofdm.hip: ofdm_tx_kernel); row r equals
    ofdm_tx(iq2d[r], ...).  An nc that is not a power of two in 64 ... 4096 runs ofdm_tx_host row by row."""
    nf, nc, npb, ncp = _ofdm_check("ofdm_tx", nf, nc, npb, ncp)
    x = _ofdm_input(iq2d, "ofdm_tx_rows", 2)
    nrow, N = x.shape[0], x.shape[1] // nf
    n_out = _ffi.ofdm_tx_symbols(N, npb) * (nc + (ncp if cp else 0))
    if nrow == 0 or n_out == 0:
        return np.zeros((nrow, n_out), dtype=x.dtype)
    if not _ofdm_on_gpu(nc):
        log.info("ofdm_tx: nc = %d is not a power of two in 64 ... 4096: host float64 path", nc)
        return np.stack([ofdm_tx_host(r, nf, nc, npb, cp, ncp) for r in x])
    return _ffi.ofdm_tx_rows(np.ascontiguousarray(x[:, :N * nf]), nf, nc, npb, cp, ncp)


def ofdm_tx(iq_data, nf, nc, npb=0, cp=False, ncp=0):
    """x_out = ofdm_tx(iq_data, nf, nc, npb=0, cp=False, ncp=0), digitalcom.py:1322-1386, on the GPU: the input cut to a multiple of nf,
    pilots multiplexed in for npb > 0 (mux_pilot_blocks, its trailing zero row included), carrier c in bin c + 1 (c < nf / 2) or
    nc - nf + c, one inverse transform per symbol scaled 1 / nc, and with cp=True the last ncp samples in front of each symbol.

    Deliberate differences (tests/golden/g24_conventions.json): nothing is printed; complex64 / float32 input gives complex64 (computed in
    float64, rounded once), everything else complex128; ValueError for an odd nf, nf > nc - 2, npb = 1, npb < 0, ncp < 0 or ncp > nc; an
    input shorter than a symbol gives what the reference's arithmetic gives (empty without pilots)."""
    x = _ofdm_input(iq_data, "ofdm_tx", 1)
    return ofdm_tx_rows(x[None, :], nf, nc, npb, cp, ncp)[0]


def _rx_h_rows(npb, nrow, nf, hht, h):
    if npb > 0:
        return h
    return np.tile(hht, (nrow, 1)) if npb == -1 else np.ones((nrow, nf))


def ofdm_rx_rows(x2d, nf, nc, npb=0, cp=False, ncp=0, alpha=0.95, ht=None):
    """Beyond the reference: (z2d, H2d) = ofdm_rx of every row of a frame set (csrc/ofdm.hip: ofdm_rx_kernel and, for npb > 0, the estimator
    kernels); row r equals ofdm_rx(x2d[r], ...).  An nc that is not a power of two in 64 ... 4096 runs ofdm_rx_host row by row."""
    nf, nc, npb, ncp = _ofdm_check("ofdm_rx", nf, nc, npb, ncp, True, ht)
    x = _ofdm_input(x2d, "ofdm_rx_rows", 2)
    hht = _ofdm_hht(ht, nf, nc, "ofdm_rx")
    nrow, nsym = x.shape[0], x.shape[1] // (nc + ncp)
    n_out = _ffi.ofdm_rx_data_symbols(nsym, npb) * nf
    if nrow == 0 or nsym == 0:
        return np.zeros((nrow, n_out), dtype=x.dtype), _rx_h_rows(npb, nrow, nf, hht, np.full((nrow, nf), np.nan + 0j))
    if not _ofdm_on_gpu(nc):
        log.info("ofdm_rx: nc = %d is not a power of two in 64 ... 4096: host float64 path", nc)
        rows = [ofdm_rx_host(r, nf, nc, npb, cp, ncp, alpha, ht) for r in x]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    n_in = nsym * (nc + ncp if cp else nc)
    z, h = _ffi.ofdm_rx_rows(np.ascontiguousarray(x[:, :n_in]), nsym, nf, nc, npb, cp, ncp, alpha, hht)
    return z, _rx_h_rows(npb, nrow, nf, hht, h)


def ofdm_rx(x, nf, nc, npb=0, cp=False, ncp=0, alpha=0.95, ht=None):
    """z_out, H = ofdm_rx(x, nf, nc, npb=0, cp=False, ncp=0, alpha=0.95, ht=None), digitalcom.py:1459-1547, on the GPU.  As the reference
    computes it: len(x) // (nc + ncp) symbols also with cp=False (their stride is then nc); npb = 0: no equalisation, H = ones(nf);
    npb = -1: every symbol divided by fft(ht, nc) on the filled carriers, which is H; npb > 0 with ht: symbols k % npb == 0 are pilots and
    run the recursive estimate, the data symbols are divided by the channel of ht (not by the estimate), H is the last estimate.

    Deliberate differences (tests/golden/g24_conventions.json): npb > 0 with ht=None runs the documented intent -- data symbols divided by
    the estimate of the latest pilot in front of them -- where the reference raises; nothing is plotted; complex64 / float32 input gives
    complex64 z; ValueError for the argument errors of ofdm_tx, npb < -1, npb = -1 without ht and len(ht) > nc; an input shorter than a
    symbol gives an empty z (H as above; all nan where no pilot was seen)."""
    xin = _ofdm_input(x, "ofdm_rx", 1)
    z, H = ofdm_rx_rows(xin[None, :], nf, nc, npb, cp, ncp, alpha, ht)
    return z[0], H[0]


def chan_est_equalize(z, npbp, alpha, ht=None):
    """zz_out, H = chan_est_equalize(z, npbp, alpha, ht=None), digitalcom.py:1389-1456, on the GPU (csrc/ofdm.hip: ofdm_chanest_kernel,
    ofdm_equalize_kernel): the pilot rows k % npbp == 0 of the (N, nf) array z run H = z[0], H = alpha H + (1 - alpha) z[k] and are removed;
    the data rows are divided by ht (the channel on the nf carriers) where it is given, as in the reference, else by the estimate of the
    latest pilot in front of them (the reference's dead branch; it raises there).  H is the last estimate.  Nothing is plotted."""
    zin = _ofdm_input(z, "chan_est_equalize", 2)
    N, nf = zin.shape
    if N == 0 or nf > 4096 or nf == 0:
        return chan_est_equalize_host(zin, npbp, alpha, ht)
    if int(npbp) < 2:
        raise ValueError("chan_est_equalize: npbp must be at least 2")
    if ht is not None and np.shape(ht) != (nf,):
        raise ValueError("chan_est_equalize: ht holds the channel on the nf carriers")
    out, h = _ffi.ofdm_equalize_rows(np.ascontiguousarray(zin)[None], int(npbp), alpha, ht)
    return out[0], h[0]


# ------------------------------------------------------------------------------------------------ xcorr, qam_sep, qpsk_bep, bpsk_bep
# (digitalcom.py:1163-1179, 495-582, 723-790, 793-846).  What the reference computes, its quirks included, and the deliberate differences:
# tests/golden/g25_conventions.json, DESIGN.md 4.20.
class _SymStream:
    """A one-dimensional stream for the symbol-error tools: a host sequence (uploaded on first use) or an _ffi.DeviceArray (never copied whole)"""

    def __init__(self, v, name):
        self.owned = None
        if isinstance(v, _ffi.DeviceArray):
            self.dev, self.host, self.n, self.dtype = v, None, v.n, v.dtype
        else:
            a = _ffi._stream(v, name)
            if a.ndim != 1:
                raise ValueError("%s must be one-dimensional (got shape %r)" % (name, a.shape))
            self.dev, self.host, self.n, self.dtype = None, a, a.size, a.dtype

    def head(self, at, count):
        count = max(0, min(count, self.n - at))
        return self.host[at:at + count] if self.host is not None else self.dev.to_host(at, count)

    def ptr(self, at):
        if self.dev is None:
            self.dev = self.owned = _ffi.DeviceArray.from_host(self.host)
        return self.dev.ptr + int(at) * self.dtype.itemsize

    def free(self):
        if self.owned is not None:
            self.owned.free()
            self.owned = self.dev = None


def _sep_levels(mod):
    levels = _ffi.QAM_LEVELS.get(mod.lower()) if isinstance(mod, str) else None
    if levels is None:
        raise ValueError('Unknown mod_type')
    return levels


def _normalise(R, E1, E2, name):
    if not (np.all(np.isfinite(R.real)) and np.all(np.isfinite(R.imag)) and np.isfinite(E1) and np.isfinite(E2)):
        raise ValueError("%s: a sample is not finite" % name)
    if R.size and (E1 == 0 or E2 == 0):
        raise ValueError("%s: a stream has zero energy" % name)
    return R / np.sqrt(E1 * E2) if R.size else R


def _lag_corr_streams(a, b, at, n, n_lags, levels):
    """lagcorr_kernel on n samples of two _SymStreams from element `at`: (R, lags, E1, E2), unnormalised"""
    nl, l0 = _ffi.lag_corr_len(n, n_lags)
    lags = l0 + np.arange(nl, dtype=np.int64)
    if nl == 0:
        return np.zeros(0, dtype=np.complex128), lags, 0.0, 0.0
    out = _ffi.DeviceArray(nl + 1, np.complex128)
    try:
        _ffi.lag_corr_dev(a.ptr(at), b.ptr(at), n, n_lags, out.ptr, out.ptr + 16 * nl, levels, a.dtype, b.dtype)
        res = out.to_host()
    finally:
        out.free()
    return res[:nl], lags, float(res[nl].real), float(res[nl].imag)


def xcorr_host(x1, x2, n_lags):
    """xcorr in NumPy (no GPU), the reference's FFT form in float64 / complex128: the yardstick of xcorr."""
    x1, x2 = _SymStream(x1, "x1").host, _SymStream(x2, "x2").host
    K = 2 * (x1.size // 2)
    if x2.size < K or int(n_lags) != n_lags or n_lags < 0:
        raise ValueError("xcorr: x2 must hold at least K = %d samples and n_lags be a non-negative integer" % K)
    a, b = x1[:K].astype(np.complex128), x2[:K].astype(np.complex128)
    k = np.arange(K) - K // 2
    keep = np.abs(k) <= n_lags
    R = np.fft.fftshift(np.fft.ifft(np.fft.fft(a) * np.conj(np.fft.fft(b)))) if K else np.zeros(0, dtype=np.complex128)
    return _normalise(R[keep], float(np.sum(np.abs(a) ** 2)), float(np.sum(np.abs(b) ** 2)), "xcorr"), k[keep]


def xcorr(x1, x2, n_lags):
    """r12, k = xcorr(x1, x2, n_lags), digitalcom.py:1163-1179: the energy-normalised circular cross-correlation of the first K = 2 (len(x1) // 2)
    samples, r12[i] = sum_n x1[(n + k[i]) mod K] conj(x2[n]) / sqrt(E1 E2), for the lags |k| <= n_lags behind the reference's fftshift (k from
    -K / 2 to K / 2 - 1).  The reference takes four whole-length FFTs; here only the lag window is computed, by direct float64 summation on the GPU
    (csrc/symerr.hip: lagcorr_kernel), 2e-17 from the exact value where the FFT form lies 3.5e-16 from it.  r12 is complex128, k int64.
    x1 / x2: sequences or _ffi.DeviceArray.

    Deliberate differences (tests/golden/g25_conventions.json): ValueError for a non-finite sample, a stream of zero energy (the reference returns
    nan) and an x2 shorter than K (the reference fails to broadcast)."""
    a, b = _SymStream(x1, "x1"), _SymStream(x2, "x2")
    K = 2 * (a.n // 2)
    if b.n < K or int(n_lags) != n_lags or n_lags < 0:
        raise ValueError("xcorr: x2 must hold at least K = %d samples and n_lags be a non-negative integer" % K)
    try:
        R, lags, E1, E2 = _lag_corr_streams(a, b, 0, a.n, int(n_lags), 0)
    finally:
        a.free()
        b.free()
    return _normalise(R, E1, E2, "xcorr"), lags


def _pick_rotation(R, lags, bpsk=False):
    """(kmax, taumax) from one correlation: rotation k's candidate is Re((1j)^k R) (BPSK: (-1)^k); the largest maximum, ties to the smallest k, then
    the first lag"""
    cands = [R.real, -R.real] if bpsk else [R.real, -R.imag, -R.real, R.imag]
    tops = np.array([c.max() for c in cands])
    kmax = int(np.argmax(tops))
    return kmax, int(lags[int(np.argmax(cands[kmax]))])


def _integer_valued(x):
    return bool(np.all(np.isfinite(x.real)) and np.all(np.isfinite(x.imag)) and np.all(x.real == np.rint(x.real)) and np.all(x.imag == np.rint(x.imag)))


def _exact_circular(a, b):
    """sum_n a[(n + m) mod N] conj(b[n]) of two integer-valued complex vectors of equal length as exact Gaussian integers (float64 holds them), or
    None where a float64 FFT cannot guarantee them: every value is an integer below N max|a| max|b|, the FFT's error is some 1e-15 of that"""
    N = a.size
    bound = N * (np.max(np.abs(a)) if N else 0) * (np.max(np.abs(b)) if N else 0)
    if bound >= 2.0 ** 40:
        return None
    R = np.fft.ifft(np.fft.fft(a) * np.conj(np.fft.fft(b)))
    return np.rint(R.real) + 1j * np.rint(R.imag)


def qam_sep_search(tx, rx_q, n_corr):
    """(kmax, taumax) of qam_sep's search in exact integers on the host: tx integer-valued, rx_q quantised, equal lengths."""
    K = 2 * (tx.size // 2)
    R = _exact_circular(rx_q[:K].astype(np.complex128), tx[:K].astype(np.complex128))
    if R is None:
        raise ValueError("qam_sep: streams too long or too large for the exact host search")
    k = np.arange(K) - K // 2
    keep = np.abs(k) <= n_corr
    return _pick_rotation(np.fft.fftshift(R)[keep], k[keep])


def _sep_result(count, counts, SEP_disp):
    if counts[3]:
        raise ValueError("qam_sep: %d symbols of the overlap are not finite or tx_data is not integer-valued there" % counts[3])
    errors = int(counts[0])
    if SEP_disp:
        log.info('Symbols = %d, Errors %d, SEP = %1.2e' % (count, errors, errors / float(count)))
    return count, errors, errors / float(count)


def qam_sep_host(tx_data, rx_data, mod, n_corr=1024, n_transient=0, SEP_disp=True):
    """qam_sep in NumPy (no GPU): the yardstick of qam_sep."""
    levels = _sep_levels(mod)
    n_corr, n_transient = _check_n_corr(n_corr, n_transient)
    tx, rx = _SymStream(tx_data, "tx_data").host[n_transient:], _SymStream(rx_data, "rx_data").host[n_transient:]
    n = min(tx.size, rx.size)
    if n < 2:
        raise ValueError("qam_sep: fewer than two symbols behind the transient")
    tx, rx = tx[:n].astype(np.complex128), rx[:n]
    if not (np.all(np.isfinite(rx.real)) and np.all(np.isfinite(rx.imag))):
        raise ValueError("qam_sep: a sample is not finite")
    if not _integer_valued(tx):
        raise ValueError("qam_sep: tx_data must hold integer-valued symbols (qam_bb's tx_data)")
    rq = _ffi.qam_quantise_host(rx, levels)
    if not np.any(tx[:2 * (n // 2)]) or not np.any(rq[:2 * (n // 2)]):
        raise ValueError("qam_sep: a stream has zero energy")
    kmax, taumax = qam_sep_search(tx, rq, n_corr)
    if SEP_disp:
        log.info('Phase ambiquity = (1j)**%d, taumax = %d' % (kmax, taumax))
    t0, r0, count = _overlap(n, n, taumax)
    if count <= 0:
        raise ValueError("qam_sep: the streams do not overlap at lag %d" % taumax)
    counts = _ffi.sym_count_rows_host(tx[None, t0:t0 + count], rx[None, r0:r0 + count], _ffi.SYM_QAM, levels, kmax)[0]
    return _sep_result(count, counts, SEP_disp)


def _count_streams(tx, rx, t_at, r_at, count, mode, levels, kphase):
    """symcount_kernel on one row of `count` symbols of two _SymStreams: int64[4]"""
    cnt = _ffi.DeviceBytes(32)
    try:
        _ffi.sym_count_rows_dev(tx.ptr(t_at), tx.dtype, 0, 0, rx.ptr(r_at), rx.dtype, 0, 0, 1, 0, count, 1, mode, levels, kphase, cnt)
        return cnt.read().view(np.int64)
    finally:
        cnt.free()


def qam_sep(tx_data, rx_data, mod, n_corr=1024, n_transient=0, SEP_disp=True):
    """Nsymb, Nerr, SEP_hat = qam_sep(tx_data, rx_data, mod, n_corr=1024, n_transient=0, SEP_disp=True), digitalcom.py:495-582: the soft symbols
    of rx_data (on the unit square) are quantised to the M levels of mod ('qpsk', '16qam', '64qam', '256qam'), the lag |tau| <= n_corr and the
    rotation (1j)^k between the streams are found from xcorr over the WHOLE stream, and the symbols that differ are counted over the overlap.

    The reference takes sixteen whole-length FFTs for the search.  Here the quantiser runs at the load of one lag-window correlation on the GPU
    (csrc/symerr.hip: lagcorr_kernel): quantised rx and qam_bb's tx_data are Gaussian integers, so every correlation value is an exact integer,
    rotation k's candidate is Re((1j)^k R0), and the pick is the exact maximum -- ties to the smallest k, then the first lag, as bit_errors_search.
    Only the 2 n_corr + 1 values cross to the host.  The count (quantise, rotate, compare) is one fused kernel over the overlap (symcount_kernel).
    Returns (int, int, float) and logs the reference's two lines.  tx_data / rx_data: sequences or _ffi.DeviceArray.

    Deliberate differences (tests/golden/g25_conventions.json): n_corr follows bit_errors' rules (even, at most 65536); ValueError for an unknown
    mod, a non-finite sample, a tx_data that is not integer-valued, a stream of zero energy and an empty overlap."""
    levels = _sep_levels(mod)
    n_corr, n_transient = _check_n_corr(n_corr, n_transient)
    tx, rx = _SymStream(tx_data, "tx_data"), _SymStream(rx_data, "rx_data")
    n = min(tx.n, rx.n) - n_transient
    if n < 2:
        raise ValueError("qam_sep: fewer than two symbols behind the transient")
    try:
        R, lags, E1, E2 = _lag_corr_streams(rx, tx, n_transient, n, n_corr, levels)
        _normalise(R, E1, E2, "qam_sep")
        if not _integer_valued(R):
            raise ValueError("qam_sep: tx_data must hold integer-valued symbols (qam_bb's tx_data)")
        kmax, taumax = _pick_rotation(R, lags)
        if SEP_disp:
            log.info('Phase ambiquity = (1j)**%d, taumax = %d' % (kmax, taumax))
        t0, r0, count = _overlap(n, n, taumax)
        if count <= 0:
            raise ValueError("qam_sep: the streams do not overlap at lag %d" % taumax)
        counts = _count_streams(tx, rx, n_transient + t0, n_transient + r0, count, _ffi.SYM_QAM, levels, kmax)
    finally:
        tx.free()
        rx.free()
    return _sep_result(count, counts, SEP_disp)


def bep_search(tx_head, rx_head, n_corr, bpsk=False, exact=True):
    """(kmax, taumax) of qpsk_bep's / bpsk_bep's search: the length-n_corr circular correlation of the two heads (cut or zero-padded to n_corr),
    lag 0 at n_corr / 2 behind the fftshift.  Integer-valued heads: exact integers, one correlation, the candidates Re((1j)^k R0) (BPSK: +-Re R0),
    ties to the smallest k, then the first lag.  Otherwise (or with exact=False) the reference's own float64 FFT expression per rotation."""
    def fit(v):
        out = np.zeros(n_corr, dtype=np.float64 if bpsk else np.complex128)
        v = np.asarray(v)[:n_corr]
        out[:v.size] = v.real if bpsk else v
        return out
    t, r = fit(tx_head), fit(rx_head)
    if not (np.all(np.isfinite(t.real)) and np.all(np.isfinite(t.imag)) and np.all(np.isfinite(r.real)) and np.all(np.isfinite(r.imag))):
        raise ValueError("%s: a sample is not finite" % ("bpsk_bep" if bpsk else "qpsk_bep"))
    lags = np.arange(n_corr) - n_corr // 2
    R = _exact_circular(r, t) if exact and _integer_valued(t) and _integer_valued(r) else None
    if R is not None:
        return _pick_rotation(np.fft.fftshift(R), lags, bpsk)
    T = np.conj(np.fft.fft(t, n_corr))
    rots = (1, -1) if bpsk else (1, 1j, -1, -1j)
    cands = [np.fft.fftshift(np.fft.ifft(np.fft.fft(r if k == 0 else rot * r, n_corr) * T)).real for k, rot in enumerate(rots)]
    kmax = int(np.argmax(np.array([c.max() for c in cands])))
    return kmax, int(lags[int(np.argmax(cands[kmax]))])


def _bep(name, mode, host, tx_data, rx_data, n_corr, n_transient):
    n_corr, n_transient = _check_n_corr(n_corr, n_transient)
    tx, rx = _SymStream(tx_data, "tx_data"), _SymStream(rx_data, "rx_data")
    n_tx, n_rx = tx.n - n_transient, rx.n - n_transient
    if n_tx <= 0 or n_rx <= 0:
        raise ValueError("%s: no symbols behind the transient" % name)
    kmax, taumax = bep_search(tx.head(n_transient, n_corr), rx.head(n_transient, n_corr), n_corr, mode == _ffi.SYM_BPSK)
    log.info('kmax =  %d, taumax = %d' % (kmax, taumax))
    t0, r0, count = _overlap(n_tx, n_rx, taumax)
    try:
        if count <= 0:
            counts = np.zeros(4, dtype=np.int64)
        elif host:
            counts = _ffi.sym_count_rows_host(tx.host[None, n_transient + t0:n_transient + t0 + count], rx.host[None, n_transient + r0:n_transient + r0 + count], mode, 0, kmax)[0]
        else:
            counts = _count_streams(tx, rx, n_transient + t0, n_transient + r0, count, mode, 0, kmax)
    finally:
        tx.free()
        rx.free()
    if counts[3]:
        raise ValueError("%s: %d symbols of the overlap are not finite or beyond int16 as (v + 1) / 2" % (name, counts[3]))
    return max(count, 0), counts


def qpsk_bep(tx_data, rx_data, n_corr=1024, n_transient=0):
    """S_count, I_errors, Q_errors, S_errors = qpsk_bep(tx_data, rx_data, n_corr=1024, n_transient=0), digitalcom.py:723-790: lag and rotation
    (1j)^k from the first n_corr symbols behind the transient (bep_search, on the host: only 2 n_corr elements leave the device), then over the
    whole overlap tI = int16((re tx + 1) / 2), rI likewise of the rotated rx, the same for Q, and sum(tI ^ rI), sum(tQ ^ rQ),
    sum((tI ^ rI) | (tQ ^ rQ)) on the GPU (csrc/symerr.hip: symcount_kernel) -- the reference's integers also where soft values make them other
    than 0 / 1.  Returns (int, numpy.int64, numpy.int64, numpy.int64).  tx_data / rx_data: sequences or _ffi.DeviceArray.

    Deliberate differences (tests/golden/g25_conventions.json): the reference raises TypeError on every call with NumPy 2 (its float taumax is
    used as a slice index); this builds the documented intent, int(taumax), as bpsk_bep does.  n_corr follows bit_errors' rules; ValueError for a
    non-finite sample and for |(v + 1) / 2| >= 32768; integer-valued heads are searched in exact integers (ties: smallest k, first lag)."""
    count, c = _bep("qpsk_bep", _ffi.SYM_QPSK, False, tx_data, rx_data, n_corr, n_transient)
    return count, c[0], c[1], c[2]


def qpsk_bep_host(tx_data, rx_data, n_corr=1024, n_transient=0):
    """qpsk_bep in NumPy (no GPU): the yardstick of qpsk_bep."""
    count, c = _bep("qpsk_bep", _ffi.SYM_QPSK, True, tx_data, rx_data, n_corr, n_transient)
    return count, c[0], c[1], c[2]


def bpsk_bep(tx_data, rx_data, n_corr=1024, n_transient=0):
    """S_count, S_errors = bpsk_bep(tx_data, rx_data, n_corr=1024, n_transient=0), digitalcom.py:793-846: as qpsk_bep on the real parts with the
    sign (-1)^k; S_errors = sum(int16((tx + 1) / 2) ^ int16((rx + 1) / 2)) over the overlap, numpy.int64."""
    count, c = _bep("bpsk_bep", _ffi.SYM_BPSK, False, tx_data, rx_data, n_corr, n_transient)
    return count, c[0]


def bpsk_bep_host(tx_data, rx_data, n_corr=1024, n_transient=0):
    """bpsk_bep in NumPy (no GPU): the yardstick of bpsk_bep."""
    count, c = _bep("bpsk_bep", _ffi.SYM_BPSK, True, tx_data, rx_data, n_corr, n_transient)
    return count, c[0]


def _sym_rows(name, fn, tx2d, rx2d, mode, levels, kphase, start, step):
    counts = fn(tx2d, rx2d, mode, levels, kphase, start, step)
    if np.any(counts[:, 3]):
        raise ValueError("%s: %d symbols break a precondition (not finite, tx not integer-valued, or beyond int16 as (v + 1) / 2)" % (name, int(counts[:, 3].sum())))
    tx, rx = np.asarray(tx2d), np.asarray(rx2d)
    return min(tx.shape[1], _ffi.sym_count(rx.shape[1], start, step)), counts


def qam_sep_rows(tx2d, rx2d, mod, kphase=0, start=0, step=1):
    """Beyond the reference: (symbols_per_row, errors int64[nrow]) of aligned rows, no search, one launch of the fused count (csrc/symerr.hip):
    row r's rx symbols rx2d[r, start::step], quantised to mod's levels and rotated by (1j)^kphase, against tx2d[r, :].  Mirrors bit_errors_rows."""
    n, c = _sym_rows("qam_sep_rows", _ffi.sym_count_rows, tx2d, rx2d, _ffi.SYM_QAM, _sep_levels(mod), kphase, start, step)
    return n, c[:, 0].copy()


def qam_sep_rows_host(tx2d, rx2d, mod, kphase=0, start=0, step=1):
    """qam_sep_rows in NumPy (no GPU)."""
    n, c = _sym_rows("qam_sep_rows", _ffi.sym_count_rows_host, tx2d, rx2d, _ffi.SYM_QAM, _sep_levels(mod), kphase, start, step)
    return n, c[:, 0].copy()


def qpsk_bep_rows(tx2d, rx2d, kphase=0, start=0, step=1):
    """Beyond the reference: (symbols_per_row, I_errors, Q_errors, S_errors), each int64[nrow], of aligned rows in one launch."""
    n, c = _sym_rows("qpsk_bep_rows", _ffi.sym_count_rows, tx2d, rx2d, _ffi.SYM_QPSK, 0, kphase, start, step)
    return n, c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()


def qpsk_bep_rows_host(tx2d, rx2d, kphase=0, start=0, step=1):
    """qpsk_bep_rows in NumPy (no GPU)."""
    n, c = _sym_rows("qpsk_bep_rows", _ffi.sym_count_rows_host, tx2d, rx2d, _ffi.SYM_QPSK, 0, kphase, start, step)
    return n, c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()


def bpsk_bep_rows(tx2d, rx2d, kphase=0, start=0, step=1):
    """Beyond the reference: (symbols_per_row, S_errors int64[nrow]) of aligned rows in one launch."""
    n, c = _sym_rows("bpsk_bep_rows", _ffi.sym_count_rows, tx2d, rx2d, _ffi.SYM_BPSK, 0, kphase, start, step)
    return n, c[:, 0].copy()


def bpsk_bep_rows_host(tx2d, rx2d, kphase=0, start=0, step=1):
    """bpsk_bep_rows in NumPy (no GPU)."""
    n, c = _sym_rows("bpsk_bep_rows", _ffi.sym_count_rows_host, tx2d, rx2d, _ffi.SYM_BPSK, 0, kphase, start, step)
    return n, c[:, 0].copy()
