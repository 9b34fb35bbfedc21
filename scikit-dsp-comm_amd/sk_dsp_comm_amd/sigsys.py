"""Rate-change and CIC-tap primitives with the signatures of sk_dsp_comm.sigsys.

  upsample(x, L)       /root/reference/src/sk_dsp_comm/sigsys.py:3031-3053
  downsample(x, M, p)  /root/reference/src/sk_dsp_comm/sigsys.py:3056-3083
  cic(m, k)            /root/reference/src/sk_dsp_comm/sigsys.py:62-93

  os_filter(x,h,N,mode) /root/reference/src/sk_dsp_comm/sigsys.py:482-540   ("next" row)
  oa_filter(x,h,N,mode) /root/reference/src/sk_dsp_comm/sigsys.py:543-598

Callers around the hot path, same signatures, the filtering on the GPU:
  interp24(x) / deci24(x)         sigsys.py:2945-3028   3-stage (b,a) Butterworth x24 / /24
  ten_band_eq_filt(x, GdB, Q)     sigsys.py:96-141      ten peaking biquads -> one SOS scan
  peaking(GdB, fc, Q, fs)         sigsys.py:202-260     (host design)
  rc_imp / sqrt_rc_imp            sigsys.py:1847-1945   (host pulse design)
  nrz_bits / nrz_bits2            sigsys.py:2120-2211   lfilter(b, 1, zero-stuffed data) -> polyphase .up
  fft_filt_bank(x, h, ...)        sigsys.py:2588-2694   (8f-4) one FIR per band with frequency-shifted taps
  fft_caf(x, h_ref, ...)          sigsys.py:2696-2781   streaming cross-ambiguity function: all frequency slices from ONE pass
                                                        over the input (csrc/fir_bank.hip); fft_caf_host: its float64 host restatement

Spectrum estimation, one GPU primitive (csrc/psd.hip: windowed overlapping FFTs in LDS, |X|^2 summed in float64):
  psd(x, n_fft, fs, overlap_percent, scale_noise)  sigsys.py:2497-2585   Welch, Hann window -> (Px, f)
  my_psd(x, n_fft, fs)                             sigsys.py:2457-2494   mlab.psd defaults -> (Px, f)
  simple_sa(x, NS, NFFT, fs, NAVG, window)         sigsys.py:1008-1084   zero-padded subrecords -> (f, Sx)

upsample/downsample run on the GPU (resample.hip) and are bit-exact index moves; cic
is host-side coefficient generation (a few dozen float64 taps) and stays in NumPy.
Error conventions follow the reference (tests/golden/g10_conventions.json).
"""
from logging import getLogger

import numpy as np

from . import _ffi
from . import config

log = getLogger(__name__)


def _gpu_dtype(x):
    """Map an input array to one of the four device dtypes (value-preserving)."""
    dt = x.dtype
    if dt in (np.float32, np.complex64, np.float64, np.complex128):
        return x
    if np.issubdtype(dt, np.complexfloating):
        return x.astype(np.complex128)
    if dt == np.float16:
        return x.astype(np.float32)
    return x.astype(np.float64)  # integers / bool: what the reference's promotion gives


def cic(m, k):
    """FIR taps of k cascaded length-m boxcars with unit DC gain (sigsys.py:62-93)."""
    box = np.ones(m)
    taps = box
    for _ in range(1, k):                 # k <= 1 (0 included) leaves a single boxcar, as in the reference
        taps = np.convolve(taps, box)     # exact: the entries are integer path counts far below 2^53
    return taps / np.sum(taps)


def upsample(x, L):
    """Insert L-1 zeros between samples: y[n*L] = x[n] (sigsys.py:3050-3053).

    Like the reference the stuffing factor is int(L-1)+1 and the result is
    float64/complex128 (the reference hstacks with a float64 zeros matrix)."""
    if not hasattr(x, "reshape"):
        raise AttributeError("'%s' object has no attribute 'reshape'" % type(x).__name__)
    n_in = len(x)
    if x.ndim != 1:
        raise ValueError("cannot reshape array of size %d into shape (%d,1)" % (x.size, n_in))
    Lz = int(L - 1)
    if Lz < 0:
        raise ValueError("negative dimensions are not allowed")
    Li = Lz + 1
    out_dt = np.result_type(x.dtype, np.float64)
    if n_in == 0:
        return np.zeros(0, dtype=out_dt)
    xg = np.ascontiguousarray(_gpu_dtype(x))
    if config.strict_dtype and xg.dtype != out_dt:
        xg = xg.astype(out_dt)  # widen the n inputs, not the n*L outputs: the move itself is exact
    return _ffi.upsample(xg, Li)


def downsample(x, M, p=0):
    """Keep every M-th sample starting at phase p: y[k] = x[k*M+p] (sigsys.py:3078-3083).

    Returns a fresh contiguous array (the reference returns a strided view of x; the
    values are identical)."""
    if not isinstance(M, int):
        raise TypeError("M must be an int")
    if not hasattr(x, "reshape"):
        raise AttributeError("'%s' object has no attribute 'reshape'" % type(x).__name__)
    nk = int(np.floor(len(x) / M))  # ZeroDivisionError for M == 0, like the reference
    if x.ndim != 1:
        raise ValueError("cannot reshape array of size %d into shape (%d,%d)" % (x.size, nk, M))
    if not (-M <= p < M):
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (p, M))
    p = int(p) % M
    if nk == 0:
        return np.zeros(0, dtype=x.dtype)
    src = np.ascontiguousarray(x)
    # a pure element move: run it on the bit pattern (4/8/16-byte elements map to f32/f64/c128)
    isz = src.dtype.itemsize
    if isz == 4:
        y = _ffi.downsample(src.view(np.float32), M, p).view(src.dtype)
    elif isz == 8:
        y = _ffi.downsample(src.view(np.float64), M, p).view(src.dtype)
    elif isz == 16:
        y = _ffi.downsample(src.view(np.complex128), M, p).view(src.dtype)
    else:  # 1- and 2-byte elements: widen exactly, move, narrow
        wide = src.astype(np.float32 if src.dtype == np.float16 else np.int32)
        y = _ffi.downsample(wide.view(np.float32), M, p).view(wide.dtype).astype(src.dtype)
    return y


def _transform_domain_fir(x, h, N, mode, name):
    """Shared body of os_filter / oa_filter: both return real(lfilter(h, 1, x)) as float64
    (the reference takes np.real of every inverse FFT frame).  The frame size N only
    parameterises the reference's Python frame loop; here the filtering runs in the GPU
    overlap-save engine (fir_ols.hip) with its own 8192-point tiles."""
    from . import multirate_helper as mrh
    P = len(h)
    L = int(N) - P + 1
    if L <= 0:
        raise ValueError("%s: FFT size N=%d must exceed the filter length P=%d - 1" % (name, int(N), P))
    x = np.asarray(x)
    if len(x) == 0:
        return (np.zeros(0), np.zeros((0, 0))) if mode == 1 else np.zeros(0)
    y = mrh.multirate_FIR(np.asarray(h))._filter(x, True)   # the reference's float64 / complex128 whatever config.strict_dtype says
    y = np.ascontiguousarray(np.real(y), dtype=np.float64)
    if mode == 1:
        return y, _frame_matrix(x, np.asarray(h), int(N), name)
    return y


def _frame_matrix(x, h, N, name):
    """The diagnostic matrix of os_filter / oa_filter(mode=1): row k holds the N outputs of frame k's circular
    convolution at the frame's position (sigsys.py:517-540, 582-598).  It is a teaching aid of the reference's frame
    loop (Nframe x Nx float64 -- quadratic in the signal length), computed here on the host with one batched FFT;
    the filtered signal itself comes from the GPU."""
    P, Nx0 = len(h), len(x)
    L = N - P + 1
    H = np.fft.fft(h, N)
    if name == "os_filter":
        xp = np.concatenate([np.zeros(P - 1), x])
        Nx = len(xp)
        nframe = int(np.ceil(Nx / float(L)))
        xp = np.concatenate([xp, np.zeros(nframe * L - Nx + N)])
        frames = np.stack([xp[k * L:k * L + N] for k in range(nframe)])
    else:
        Nx = Nx0
        nframe = int(np.ceil(Nx / float(L)))
        xp = np.concatenate([x, np.zeros(nframe * L - Nx)])
        frames = xp.reshape(nframe, L)
    yk = np.real(np.fft.ifft(np.fft.fft(frames, N, axis=1) * H, axis=1))
    y_mat = np.zeros((nframe, nframe * N))
    for k in range(nframe):
        y_mat[k, k * L:k * L + N] = yk[k]
    return y_mat[:, P - 1:Nx] if name == "os_filter" else y_mat[:, 0:Nx]


def os_filter(x, h, N, mode=0):
    """Overlap-and-save FIR filtering (sigsys.py:482-540): y = real(lfilter(h, 1, x))."""
    return _transform_domain_fir(x, h, N, mode, "os_filter")


def oa_filter(x, h, N, mode=0):
    """Overlap-and-add FIR filtering (sigsys.py:543-598): y = real(lfilter(h, 1, x))."""
    return _transform_domain_fir(x, h, N, mode, "oa_filter")


# ---------------------------------------------------------------------------------------------
# callers around the hot path
# ---------------------------------------------------------------------------------------------
def _lfilter_dtype(x):
    """(device array, result dtype) for scipy.signal.lfilter(b, a, x) with float64 coefficients."""
    from . import multirate_helper as mrh
    return mrh._signal(np.asarray(x))


def _butter_stage(order, wn, dtype):
    import scipy.signal as signal
    b, a = signal.butter(order, wn)
    return _ffi.IirKernel(_ffi.code_of(dtype), b=b, a=a)


def interp24(x):
    """Interpolate by 24 in three stages x2, x3, x4, each lfilter(b, a, L*upsample(., L)) with a
    10th-order Butterworth at 1/L (sigsys.py:2945-2985).  One fused zero-stuff + scan per stage."""
    from . import multirate_helper as mrh
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("cannot reshape array of size %d into shape (%d,1)" % (x.size, len(x)))
    xg, ref_dt = _lfilter_dtype(x)
    if xg.size == 0:
        return np.zeros(0, dtype=ref_dt)
    y = xg
    for L in (2, 3, 4):
        y = _butter_stage(10, 1.0 / L, y.dtype).up(y, L, wide=config.strict_dtype and L == 4)
    return mrh._finish(y, ref_dt)


def deci24(x):
    """Decimate by 24 in three stages /2, /3, /4, each downsample(lfilter(b, a, .), M) with a
    10th-order Butterworth at 1/M (sigsys.py:2988-3028); only the kept samples are written."""
    from . import multirate_helper as mrh
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("deci24 expects a 1-D signal")
    xg, ref_dt = _lfilter_dtype(x)
    y = xg
    for M in (2, 3, 4):
        if len(y) // M == 0:
            return np.zeros(0, dtype=ref_dt if config.strict_dtype else xg.dtype)
        y = _butter_stage(10, 1.0 / M, y.dtype).dn(y, M, wide=config.strict_dtype and M == 4)
    return mrh._finish(y, ref_dt)


def peaking(GdB, fc, Q=3.5, fs=44100.):
    """Second-order peaking (bell) equaliser section, gain GdB at fc (sigsys.py:202-260).
    Returns (b, a) with a[0] = 1."""
    mu = 10.0 ** (GdB / 20.0)
    w0 = 2.0 * np.pi * fc / fs
    kq = 4.0 / (1.0 + mu) * np.tan(w0 / (2.0 * Q))
    c0 = np.cos(w0)
    den_b, den_a = 1.0 + kq * mu, 1.0 + kq
    b = (den_b / den_a) * np.array([1.0, -2.0 * c0 / den_b, (1.0 - kq * mu) / den_b])
    a = np.array([1.0, -2.0 * c0 / den_a, (1.0 - kq) / den_a])
    return b, a


def ten_band_eq_filt(x, GdB, Q=3.5):
    """Ten octave-spaced peaking filters (31.25 Hz ... 16 kHz at fs = 44.1 kHz) in cascade
    (sigsys.py:96-141).  The reference runs ten lfilter passes; here the ten biquads are one
    SOS cascade in a single exact scan."""
    from . import multirate_helper as mrh
    nb = len(GdB)
    if not nb == 10:
        raise ValueError("GdB length not equal to ten")
    fc = 31.25 * 2.0 ** np.arange(nb)
    sos = np.zeros((nb, 6))
    for k in range(nb):
        sos[k, :3], sos[k, 3:] = peaking(GdB[k], fc[k], Q)
    xg, ref_dt = _lfilter_dtype(x)
    if xg.size == 0:
        return np.zeros(0)
    y = _ffi.IirKernel(_ffi.code_of(xg.dtype), sos=sos).filter(xg, wide=config.strict_dtype)
    return mrh._finish(y, ref_dt)


def rc_imp(Ns, alpha, M=6):
    """Truncated raised-cosine pulse, 2*M*Ns+1 samples (sigsys.py:1847-1891)."""
    n = np.arange(-M * Ns, M * Ns + 1)
    t = n / float(Ns)
    den = 1.0 - 4.0 * (alpha * t) ** 2
    sing = den == 0
    b = np.sinc(t) * np.cos(np.pi * alpha * t) / np.where(sing, 1.0, den)
    if np.any(sing):
        b[sing] = np.pi / 4.0 * np.sinc(1.0 / (2.0 * alpha))
    return b


def sqrt_rc_imp(Ns, alpha, M=6):
    """Truncated square-root raised-cosine pulse, 2*M*Ns+1 samples (sigsys.py:1894-1945)."""
    n = np.arange(-M * Ns, M * Ns + 1)
    t = n / float(Ns)
    a = alpha
    den = 1.0 - 16.0 * a ** 2 * t ** 2
    sing = np.abs(den) <= np.finfo(np.float32).eps / 2
    b = 4.0 * a / (np.pi * np.where(sing, 1.0, den)) * (np.cos((1.0 + a) * np.pi * t)
                                                    + np.sinc((1.0 - a) * t) * (1.0 - a) * np.pi / (4.0 * a))
    if np.any(sing):
        b[sing] = 0.5 * ((1.0 + a) * np.sin((1.0 + a) * np.pi / (4.0 * a))
                         - (1.0 - a) * np.cos((1.0 - a) * np.pi / (4.0 * a))
                         + (4.0 * a) / np.pi * np.sin((1.0 - a) * np.pi / (4.0 * a)))
    return b


def _pulse(pulse, ns, alpha, m, err='pulse type must be rec, rc, or src'):
    kind = pulse.lower()
    if kind == 'rect':
        return np.ones(int(ns))
    if kind == 'rc':
        return rc_imp(ns, alpha, m)
    if kind == 'src':
        return sqrt_rc_imp(ns, alpha, m)
    raise ValueError(err)


def pulse_shape(symbols, b, ns):
    """lfilter(b, 1, upsample(symbols, ns)) -- the pulse-shaping step of nrz_bits*, the *_bb
    transmitters of digitalcom (digitalcom.py:1676, 1821) -- as ONE polyphase interpolation:
    only the ns-th of the products that do not multiply a stuffed zero is computed."""
    from . import multirate_helper as mrh
    ns = int(ns)
    sym = np.asarray(symbols)
    if sym.size == 0:
        return np.zeros(0, dtype=np.complex128 if np.iscomplexobj(sym) else np.float64)
    if ns == 1:
        return mrh.multirate_FIR(np.asarray(b, dtype=np.float64)).filter(sym)
    # multirate_FIR.up applies the interpolation gain ns to the stuffed signal; lfilter here does not
    return mrh.multirate_FIR(np.asarray(b, dtype=np.float64) / ns).up(sym.astype(np.result_type(sym.dtype, np.float64)), ns)


# ---- shaping and matched filtering over frame sets (csrc/pulse.hip) ---------------------------------------------------
_pulse_fallback_logged = set()


def _pulse_fallback(name, ntaps, rate):
    """outside the kernels' range (1 <= ns, step <= 64, at most 2049 taps) the existing engines run; said once per function"""
    if name not in _pulse_fallback_logged:
        _pulse_fallback_logged.add(name)
        log.info("%s: %d taps at rate %d is outside the row kernels' range (rate 1 ... %d, at most %d taps): the FIR engines run instead",
                 name, ntaps, rate, _ffi.PULSE_MAX_RATE, _ffi.PULSE_MAX_TAPS)


def _pulse_args(x2d, b, rate, name, rate_name):
    x = _ffi._pulse_rows(x2d, name)
    b = _ffi._pulse_taps(b)
    if int(rate) != rate or rate < 1:
        raise ValueError("%s: %s must be a positive integer" % (name, rate_name))
    return x, b, int(rate)


def pulse_shape_rows(sym2d, b, ns, scale=None):
    """Beyond the reference: pulse_shape of every row of sym2d -- scale * lfilter(b, 1, upsample(row, ns)), each row a frame from rest -- in one
    launch (csrc/pulse.hip: pulse_shape_rows_kernel).  b: real taps; rows float32 / complex64 / float64 / complex128 (integers run as float64),
    returned in the same dtype, (nrow, n ns).  scale: None or a real factor applied once behind the sum (the x / x_m of qam_gray_encode_bb, which
    NumPy computes as a multiplication by 1 / x_m).  The result equals pulse_shape_rows_host bit for bit.  Outside 1 <= ns <= 64 and 2049 taps:
    multirate_FIR.up per row (logged once at INFO), within that engine's contract."""
    x, b, ns = _pulse_args(sym2d, b, ns, "pulse_shape_rows", "ns")
    if x.shape[0] == 0 or x.shape[1] == 0:
        return np.zeros((x.shape[0], x.shape[1] * ns), dtype=x.dtype)
    if not _ffi.pulse_served(b.size, ns):
        _pulse_fallback("pulse_shape_rows", b.size, ns)
        y = np.stack([np.asarray(pulse_shape(row, b, ns)) for row in x])
        return (y if scale is None else y * np.float64(scale)).astype(x.dtype)
    return _ffi.PulseKernel(b, x.dtype).shape_rows(x, ns, scale)


def pulse_shape_rows_host(sym2d, b, ns, scale=None):
    """pulse_shape_rows in NumPy (no GPU): the kernel's arithmetic operation for operation (_ffi.pulse_shape_rows_host), the same bits."""
    x, b, ns = _pulse_args(sym2d, b, ns, "pulse_shape_rows", "ns")
    return _ffi.pulse_shape_rows_host(x, b, ns, scale)


def matched_filter_rows(x2d, b, start=0, step=1):
    """Beyond the reference: lfilter(b, 1, row)[start::step] of every row of x2d, each row a frame from rest, in one launch that computes only the
    outputs it keeps (csrc/pulse.hip: pulse_mf_rows_kernel); step = 1 is a plain FIR over the rows.  Same dtypes as pulse_shape_rows; the result,
    (nrow, len(row[start::step])), equals matched_filter_rows_host bit for bit.  Outside 1 <= step <= 64 and 2049 taps: multirate_FIR.filter over
    the rows and a slice (logged once at INFO), within that engine's contract."""
    x, b, step = _pulse_args(x2d, b, step, "matched_filter_rows", "step")
    if int(start) != start or start < 0:
        raise ValueError("matched_filter_rows: start must be a non-negative integer")
    start = int(start)
    n_out = _ffi.sym_count(x.shape[1], start, step)
    if x.shape[0] == 0 or n_out == 0:
        return np.zeros((x.shape[0], n_out), dtype=x.dtype)
    if not _ffi.pulse_served(b.size, step):
        from . import multirate_helper as mrh
        _pulse_fallback("matched_filter_rows", b.size, step)
        y = np.asarray(mrh.multirate_FIR(b).filter(x))
        return np.ascontiguousarray(y[:, start::step]).astype(x.dtype)
    return _ffi.PulseKernel(b, x.dtype).mf_rows(x, start, step)


def matched_filter_rows_host(x2d, b, start=0, step=1):
    """matched_filter_rows in NumPy (no GPU): the kernel's arithmetic operation for operation (_ffi.pulse_mf_rows_host), the same bits."""
    x, b, step = _pulse_args(x2d, b, step, "matched_filter_rows", "step")
    if int(start) != start or start < 0:
        raise ValueError("matched_filter_rows: start must be a non-negative integer")
    return _ffi.pulse_mf_rows_host(x, b, int(start), step)


def nrz_bits2(data, Ns, pulse='rect', alpha=0.25, M=6):
    """NRZ +-1 waveform from user bits with pulse shaping (sigsys.py:2163-2211): (x, b/Ns)."""
    data = np.asarray(data)
    b = _pulse(pulse, Ns, alpha, M)
    x = pulse_shape(2 * data - 1, b, Ns)
    return x, b / float(Ns)


def nrz_bits(n_bits, ns, pulse='rect', alpha=0.25, m=6):
    """NRZ +-1 waveform from random bits (sigsys.py:2120-2160): (x, b/ns, data)."""
    data = np.random.randint(0, 2, n_bits)
    x, b = nrz_bits2(data, ns, pulse, alpha, m)
    return x, b, data


def env_det(x):
    """Ideal envelope detector: half-wave rectifier (sigsys.py:2913-2942)."""
    x = np.asarray(x)
    return np.where(x >= 0, x, 0).astype(np.float64)


def am_tx(m, a_mod, fc=75e3):
    """AM transmitter of the Chapter-17 case study (sigsys.py:2784-2819): the message is interpolated by 24 on the GPU
    (interp24), the carrier is applied on the host.  Returns (x192, t192, m24)."""
    m24 = interp24(m)
    t192 = np.arange(len(m24)) / 192.0e3
    m_max = np.max(np.abs(m24))
    x192 = (1 + a_mod * m24 / m_max) * np.cos(2 * np.pi * fc * t192)
    return x192, t192, m24


def am_rx(x192):
    """AM envelope-detector receiver (sigsys.py:2822-2866): env_det -> deci24 (GPU) -> DC removal, plus the 192 ksps
    monitor output through two passes of a 5th-order Butterworth at 5 kHz (one 10th-order cascade launch here).
    Returns (m_rx8, t8, m_rx192, x_edet192)."""
    import scipy.signal as signal
    x_edet192 = env_det(x192)
    m_rx8 = deci24(x_edet192)
    m_rx8 = m_rx8 - np.mean(m_rx8)
    t8 = np.arange(len(m_rx8)) / 8.0e3
    b192, a192 = signal.butter(5, 2 * 5.0e3 / 192.0e3)
    if len(x_edet192):
        sos = _ffi.tf2sos(b192, a192)
        from . import multirate_helper as mrh
        m_rx192 = mrh.multirate_IIR(np.vstack([sos, sos])).filter(x_edet192)   # lfilter(b, a, lfilter(b, a, .))
    else:
        m_rx192 = np.zeros(0)
    m_rx192 = m_rx192 - np.mean(m_rx192) if len(m_rx192) else m_rx192
    return m_rx8, t8, m_rx192, x_edet192


def _band_walk(x_use, cdt, band_taps, n_tot, y):
    """Rows y[j, :len(x_use)] = lfilter(band_taps(j), 1, x_use), j < n_tot: one complex-tap FIR handle and one pass of the existing
    engines (fir_ols.hip / fir_ols64.hip / fir_direct.hip) per band over ONE device-resident input of dtype cdt; the bands in
    batches of rows of one device block (2 GiB at most), one copy back per batch."""
    n_use = len(x_use)
    xd = _ffi.DeviceArray.from_host(np.ascontiguousarray(x_use, dtype=cdt))
    per = max(1, min(n_tot, (2 << 30) // max(n_use * np.dtype(cdt).itemsize, 1)))
    yd = _ffi.DeviceArray(n_use * per, cdt)
    try:
        for j0 in range(0, n_tot, per):
            rows = min(per, n_tot - j0)
            for j in range(rows):
                _ffi.FirKernel(band_taps(j0 + j), _ffi.code_of(cdt)).filter_dev(xd, yd.window(j * n_use, n_use))
            y[j0:j0 + rows, :n_use] = yd.to_host(0, rows * n_use).reshape(rows, n_use)
    finally:
        xd.free()
        yd.free()


def fft_filt_bank(x_in, h_filt, n_fft2=512, n_bands2=0, bs=0.2, fs=1.0, n_band_odd=True):
    """Streaming filter bank of 2*n_bands2+1 (or 2*n_bands2) bands spaced by ~bs Hz
    (sigsys.py:2588-2694).  The reference overlap-saves with a 2*n_fft2 FFT and rolls H by whole
    bins per band; rolling H by s bins IS the filter h[n]*exp(j*2*pi*s*n/(2*n_fft2)), so every band
    is one complex-tap FIR over the same device-resident input (fir_ols.hip / fir_direct.hip).
    Like the reference only whole blocks of n_fft2 samples are produced; the tail stays zero.
    Returns (y_filt_bank[bands, len(x)], freq_axis, freq_axis_desired)."""
    h_filt = np.asarray(h_filt)
    if len(h_filt) > n_fft2:
        raise ValueError('Error: Must have Nfft2 = %d >= %d = len(h_ref)' % (n_fft2, len(h_filt)))
    x_in = np.asarray(x_in)
    n_x = len(x_in)
    if n_band_odd:
        n_tot = 2 * n_bands2 + 1
        step = int(round(bs * 2 * n_fft2 / fs))
        shifts = [j * step - n_bands2 * step for j in range(n_tot)]
    else:
        n_tot = 2 * n_bands2
        step = int(round(bs / 2 * 2 * n_fft2 / fs))
        shifts = [j * 2 * step - (2 * n_bands2 - 1) * step for j in range(n_tot)]
    bs_actual = step * fs / (2 * n_fft2)
    print('N_band_step = %d' % (step,))
    print('N_band_step = %d and BS_Hz_actual = %3.2f Hz' % (step, bs_actual))
    print('N_bands_tot = %d and span_Hz = +/- %4.2f Hz' % (n_tot, n_bands2 * bs_actual))
    y = np.zeros((n_tot, n_x), dtype=complex)
    n_use = (n_x // n_fft2) * n_fft2
    if n_use and n_tot:
        single = x_in.dtype in (np.float32, np.complex64) and not config.strict_dtype
        n = np.arange(len(h_filt))
        _band_walk(x_in[:n_use], np.complex64 if single else np.complex128,
                   lambda j: h_filt * np.exp(2j * np.pi * shifts[j] * n / (2 * n_fft2)), n_tot, y)
    if n_band_odd:
        freq_axis = np.arange(-n_bands2 * step, n_bands2 * step + step, step) * fs / 2 / n_fft2
        freq_axis_desired = np.rint(freq_axis / bs) * bs
    else:
        freq_axis = np.arange(-(2 * n_bands2 - 1) * step, n_bands2 * step + 2 * (step + 1), 2 * step) * fs / 2 / n_fft2
        freq_axis_desired = np.rint(freq_axis / (bs / 2)) * (bs / 2)
    return y, freq_axis, freq_axis_desired


# ---- streaming cross-ambiguity function (sigsys.py:2696-2781) ---------------------------------------------------------------
_CAF_BANK_MAX_TAPS = 2049          # csrc/fir_bank.hip: half a 4096-point tile of overlap
_CAF_BANK_TABLE_CAP = 256 << 20    # bytes of band tables one bank handle may hold (skdsp_fir_bank_create)


def _caf_band_taps(g, shift, period):
    """g[n] exp(2j pi shift n / period) with the phase reduced in integers, (shift n) mod period, before any sine or cosine:
    the filter whose period-point spectrum is np.roll(np.fft.fft(g, period), shift), for any integer shift."""
    r = (int(shift) % int(period)) * np.arange(len(g), dtype=np.int64) % int(period)
    return np.asarray(g) * np.exp(2j * np.pi * r / int(period))


def _caf_setup(x_in, h_ref, n_fft2, n_slice2, bs, fs):
    """The reference's checks, prints and integer parameters: (x, g, shifts, n_use, freq_axis, time_axis)."""
    if len(h_ref) > n_fft2:
        raise ValueError('Error: Must have Nfft2 = %d >= %d = len(h_ref)' % (n_fft2, len(h_ref)))
    n_x = len(x_in)
    n_tot = 2 * n_slice2 + 1
    step = round(bs * 2 * n_fft2 / fs)
    bs_actual = step * fs / (2 * n_fft2)
    print('N_slice_step = %d and BS_Hz_actual = %3.2fHz' % (step, bs_actual))
    print('N_slice_tot = %d and span_Hz = +/- %3.2fHz' % (n_tot, n_slice2 * bs_actual))
    n_use = (n_x // n_fft2) * n_fft2
    if n_use and not isinstance(x_in, np.ndarray):
        x_in = x_in + 0j          # the reference's own statement inside its block loop: a list or tuple raises TypeError here
    x = np.asarray(x_in)
    if x.ndim != 1:
        raise ValueError("fft_caf: x_in must be one-dimensional (got shape %r)" % (x.shape,))
    g = np.conj(np.asarray(h_ref)[::-1])      # conjugate and reverse: correlation
    shifts = [(j - n_slice2) * step for j in range(n_tot)]
    freq_axis = np.arange(-n_slice2 * step, n_slice2 * step + step, step) * fs / 2 / n_fft2
    time_axis = np.arange(0, n_x) / fs
    return x, g, shifts, n_use, freq_axis, time_axis


def _caf_rows(x_use, g, shifts, period, y):
    """The device work of fft_caf: y[j, :len(x_use)] = lfilter(_caf_band_taps(g, shifts[j], period), 1, x_use) for every slice j.

    float32 / complex64 signals (config.strict_dtype off), and every signal under config.precision == "single", with at most
    2049 reference samples: the fused bank kernel (csrc/fir_bank.hip) -- the input is read and transformed once per tile for all
    slices.  Everything else (float64 / complex128 signals, longer references, precision "double", strict_dtype): one pass of the
    existing FIR engines per slice (_band_walk), in complex64 for float32 / complex64 signals with strict_dtype off, else complex128."""
    n_use, n_tot, P = len(x_use), len(shifts), len(g)
    single_in = x_use.dtype in (np.float32, np.complex64)
    bank = P <= _CAF_BANK_MAX_TAPS and config.precision != "double" and ((single_in and not config.strict_dtype) or config.precision == "single")
    if not bank:
        cdt = np.complex64 if single_in and not config.strict_dtype and config.precision != "double" else np.complex128
        log.info("fft_caf: %d slices of %d taps over %s input through one FIR pass per slice (%s)", n_tot, P, x_use.dtype, np.dtype(cdt))
        _band_walk(x_use, cdt, lambda j: _caf_band_taps(g, shifts[j], period), n_tot, y)
        return
    sdt = np.complex64 if np.iscomplexobj(x_use) else np.float32
    xd = _ffi.DeviceArray.from_host(np.ascontiguousarray(x_use, dtype=sdt))
    # the slices in batches of rows of ONE device block (2 GiB at most) and one handle's table budget, one copy back per batch
    per = max(1, min(n_tot, (2 << 30) // (n_use * 8), _CAF_BANK_TABLE_CAP // (32768 + 16 * P)))
    yd = _ffi.DeviceArray(n_use * per, np.complex64)
    try:
        for j0 in range(0, n_tot, per):
            rows = min(per, n_tot - j0)
            _ffi.FirBank(g, shifts[j0:j0 + rows], period, sdt).filter_dev(xd, yd, n_use)
            y[j0:j0 + rows, :n_use] = yd.to_host(0, rows * n_use).reshape(rows, n_use)
    finally:
        xd.free()
        yd.free()


def fft_caf(x_in, h_ref, n_fft2=1024, n_slice2=0, bs=0.1, fs=1.0):
    """Streaming cross-ambiguity function with 2*n_slice2+1 frequency slices centred on f = 0 (sigsys.py:2696-2781).

    The reference overlap-saves with a 2*n_fft2 FFT and rolls the spectrum of g = conj(h_ref[::-1]) by s_j = (j - n_slice2) * step
    bins per slice, step = round(bs*2*n_fft2/fs).  Rolling by s_j bins IS the filter g_j[n] = g[n] exp(2j pi s_j n / (2 n_fft2)), and
    the kept half of each block holds no circular wrap because len(h_ref) <= n_fft2, so
        y[j, m] = sum_{n < len(h_ref)} g_j[n] x[m - n],  x[< 0] = 0,  m < (len(x) // n_fft2) * n_fft2;   y[j, m] = 0 beyond
    which is what runs here: all slices off ONE pass over the device-resident input (csrc/fir_bank.hip) for float32 / complex64
    signals with config.strict_dtype off and for every signal under config.precision == "single" (within 1e-6 of each row's peak);
    one FIR pass per slice on the existing engines otherwise (float64 / complex128 signals: 1e-12; logged at INFO).
    Returns (y_caf_stream[2*n_slice2+1, len(x_in)] complex128, freq_axis, time_axis) and prints the reference's two lines.
    Deliberate differences: a non-finite sample stays inside the len(h_ref) outputs per row that multiply it (the reference's
    FFT form spreads it over the whole 2*n_fft2 block of every slice), and x_in must be one-dimensional (the reference returns a
    meaningless (slices, 2) array for 2-D input): tests/golden/g17_conventions.json."""
    x, g, shifts, n_use, freq_axis, time_axis = _caf_setup(x_in, h_ref, n_fft2, n_slice2, bs, fs)
    y = np.zeros((len(shifts), len(x)), dtype=complex)
    if n_use and len(g):
        _caf_rows(_gpu_dtype(x[:n_use]), g, shifts, 2 * n_fft2, y)
    return y, freq_axis, time_axis


def fft_caf_host(x_in, h_ref, n_fft2=1024, n_slice2=0, bs=0.1, fs=1.0):
    """Host float64 restatement of fft_caf: the reference's block-FFT form (sigsys.py:2752-2777) with all blocks of a slice in one
    batched transform -- overlap-save on blocks of 2*n_fft2 samples, the spectrum of conj(h_ref[::-1]) rolled by whole bins per slice,
    the upper half of every block kept.  Same arguments, checks, printed lines and return value as fft_caf."""
    x, g, shifts, n_use, freq_axis, time_axis = _caf_setup(x_in, h_ref, n_fft2, n_slice2, bs, fs)
    y = np.zeros((len(shifts), len(x)), dtype=complex)
    if n_use and len(g):
        F = int(n_fft2)
        K = n_use // F
        xp = np.concatenate([np.zeros(F, dtype=complex), x[:n_use].astype(complex)])
        it = xp.itemsize
        blocks = np.lib.stride_tricks.as_strided(xp, shape=(K, 2 * F), strides=(F * it, it), writeable=False)
        X = np.fft.fft(blocks, axis=1)
        H = np.fft.fft(g, 2 * F)
        for j, s in enumerate(shifts):
            y[j, :n_use] = np.fft.ifft(np.roll(H, s) * X, axis=1)[:, F:].reshape(n_use)
    return y, freq_axis, time_axis


# ---- spectrum estimation: psd, my_psd, simple_sa (sigsys.py:2497-2585, 2457-2494, 1008-1084) -------------------------------
def _psd_served(n_fft):
    """What csrc/psd.hip serves: powers of two from 64 to 4096."""
    return 64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0


def psd_accum_host(x, window, n_fft, step, nseg):
    """Host float64 restatement of the Welch primitive (vectorised NumPy, any n_fft >= len(window)):
    S[k] = sum_{i < nseg} |FFT_{n_fft}(window * x[i step : i step + len(window)])[k]|^2,  k < n_fft."""
    w = np.asarray(window, dtype=np.float64)
    ns = w.size
    xd = np.ascontiguousarray(x, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    if nseg < 1 or step < 1 or (nseg - 1) * step + ns > xd.size or not 1 <= ns <= n_fft:
        raise ValueError("psd: %d segments of %d samples, %d apart, do not fit %d samples" % (nseg, ns, step, xd.size))
    S = np.zeros(n_fft)
    it = xd.itemsize
    blk = max(1, (1 << 21) // n_fft)
    for i0 in range(0, nseg, blk):
        k = min(blk, nseg - i0)
        seg = np.lib.stride_tricks.as_strided(xd[i0 * step:], shape=(k, ns), strides=(step * it, it), writeable=False)
        X = np.fft.fft(seg * w, n_fft, axis=1)
        S += (X.real ** 2 + X.imag ** 2).sum(axis=0)
    return S


def _psd_accum(x, window, n_fft, step, nseg):
    """The primitive for a one-dimensional array: on the GPU where csrc/psd.hip serves n_fft, else the host restatement."""
    if not _psd_served(n_fft):
        log.info("psd: n_fft = %d is not a power of two in 64 ... 4096: host float64 path", n_fft)
        return psd_accum_host(x, window, n_fft, step, nseg)
    xg = _gpu_dtype(x)
    if config.precision == "double" and xg.dtype in (np.float32, np.complex64):
        xg = xg.astype(np.result_type(xg.dtype, np.float64))
    elif config.precision == "single" and xg.dtype in (np.float64, np.complex128):
        xg = xg.astype(np.float32 if xg.dtype == np.float64 else np.complex64)
    used = (nseg - 1) * step + len(window)
    xg = np.ascontiguousarray(xg[:used])
    if config.precision == "single":   # float32 LDS image: the 1e-6 contract, faster for long transforms
        with _ffi.option("psd_f32_image", 1):
            return _ffi.psd_accum(xg, window, n_fft, step, nseg)
    return _ffi.psd_accum(xg, window, n_fft, step, nseg)


def _psd_input(x, name):
    """The input as a one-dimensional array (deliberate: the reference's behaviour for other shapes is an accident of
    broadcasting, tests/golden/g16_conventions.json)."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("%s: x must be one-dimensional (got shape %r)" % (name, x.shape))
    if x.dtype.kind not in "biufc":
        raise TypeError("%s: x must be numeric (got dtype %s)" % (name, x.dtype))
    return x


def _psd_segments(Q, n_fft, overlap_percent):
    """(step, K) of psd: the hop n_fft - round(overlap_percent/100 n_fft) and the number of passes of the reference's loop
    `while i*step + 1 + n_fft <= Q` (sigsys.py:2570)."""
    step = n_fft - int(np.round(overlap_percent / 100 * n_fft))
    if n_fft < 1 or step <= 0:
        raise ValueError("psd: overlap_percent = %r leaves no positive hop for n_fft = %d" % (overlap_percent, n_fft))
    return step, ((Q - 1 - n_fft) // step + 1 if Q > n_fft else 0)


def psd(x, n_fft, fs=1, overlap_percent=50, scale_noise=True):
    """Averaged periodogram (Welch) power spectral density estimate with a Hann window (sigsys.py:2497-2585).

    K = number of segments of n_fft samples, n_fft - round(overlap_percent/100 n_fft) apart, that the reference's loop
    condition i*step + 1 + n_fft <= len(x) admits (a record of exactly n_fft samples gives K = 0 and, like the reference,
    an all-nan result).  scale_noise=True scales by 1/(K U n_fft) (white noise reads its variance), False by
    1/(K n_fft^2 U2^2) (a bin-centred sinusoid reads its power).  Real x: n_fft//2 + 1 bins from 0 to fs/2; complex x:
    n_fft bins from -fs/2.  Returns (Px, f), float64.  The segment transforms and their sum run on the GPU (csrc/psd.hip)
    for n_fft a power of two in 64 ... 4096, else in the host restatement (psd_accum_host; logged at INFO).
    Deliberate differences: an overlap_percent that leaves no positive hop raises ValueError (the reference never
    terminates), and x must be one-dimensional."""
    from scipy.signal import windows
    n_fft = int(n_fft)
    step, _ = _psd_segments(0, n_fft, overlap_percent)
    x = _psd_input(x, "psd")
    Q = len(x)
    real = np.isrealobj(x)
    w = windows.hann(n_fft)
    U = sum(w ** 2) / n_fft
    U2 = sum(w) / n_fft
    K = _psd_segments(Q, n_fft, overlap_percent)[1]
    S = _psd_accum(x, w, n_fft, step, K) if K > 0 else np.zeros(n_fft)
    if real:
        Px = S[:int(n_fft / 2) + 1].copy()
        f = fs * np.arange(0, int(n_fft / 2 + 1)) / n_fft
    else:
        Px = np.hstack((S[int(n_fft / 2):], S[0:int(n_fft / 2)]))
        f = fs * np.arange(-int(n_fft / 2), int(n_fft / 2)) / n_fft
    if scale_noise:
        Px /= (K * U * n_fft)
    else:
        Px /= (K * n_fft ** 2 * U2 ** 2)
    return Px, f


def my_psd(x, n_fft=2 ** 10, fs=1):
    """matplotlib.mlab.psd(x, n_fft, fs) with its defaults, as two arrays (sigsys.py:2457-2494): np.hanning window, no
    overlap, K = len(x)//n_fft segments (a shorter x is zero-padded to n_fft), the mean over segments divided by
    fs sum(w^2); real x one-sided with every bin but DC (and Nyquist, n_fft even) doubled, complex x two-sided from -fs/2.
    Returns (Px, f), float64; GPU / host split as in psd."""
    n_fft = int(n_fft)
    if n_fft < 1:
        raise ValueError("my_psd: n_fft must be positive")
    x = _psd_input(x, "my_psd")
    if len(x) < n_fft:
        x = np.concatenate([_gpu_dtype(x), np.zeros(n_fft - len(x), dtype=_gpu_dtype(x[:0]).dtype)])
    real = np.isrealobj(x)
    w = np.hanning(n_fft)
    K = len(x) // n_fft
    S = _psd_accum(x, w, n_fft, n_fft, K) / K
    if real:
        nf = (n_fft + 1) // 2 if n_fft % 2 else n_fft // 2 + 1
        Px = S[:nf].copy()
        f = np.fft.fftfreq(n_fft, 1 / fs)[:nf]
        Px[1:-1 if n_fft % 2 == 0 else None] *= 2.
        if n_fft % 2 == 0:
            f[-1] *= -1
    else:
        c = (n_fft - 1) // 2 + 1 if n_fft % 2 else n_fft // 2
        Px = np.roll(S, -c)
        f = np.roll(np.fft.fftfreq(n_fft, 1 / fs), -c)
    Px /= fs
    Px /= (w ** 2).sum()
    return Px, f


def simple_sa(x, NS, NFFT, fs, NAVG=1, window='boxcar'):
    """Averaged periodogram of NAVG windowed subrecords of NS samples, each zero-padded to NFFT (sigsys.py:1008-1084):
    Sx = mean |FFT_NFFT(w x_k)|^2 / NFFT^2 with w = scipy.signal.get_window(window, NS, fftbins=False).  Only complex128
    input is two-sided (NFFT bins from -fs/2); every other dtype, complex64 included, takes the one-sided branch
    (NFFT//2 bins) as in the reference.  NAVG > len(x)//NS warns and returns (0, 0).  Returns (f, Sx), float64.
    The reference's malformed log.info('K = ', K) is not reproduced."""
    import warnings
    from scipy.signal import get_window
    if not hasattr(x, "dtype"):
        raise AttributeError("'%s' object has no attribute 'dtype'" % type(x).__name__)
    x = _psd_input(x, "simple_sa")
    Nx = len(x)
    K = int(Nx / NS)
    if NAVG > K:
        warnings.warn('NAVG exceeds number of available subrecords')
        return 0, 0
    NS, NFFT, NAVG = int(NS), int(NFFT), int(NAVG)
    if NAVG < 1:
        raise ZeroDivisionError("float division by zero")
    if NS > NFFT:
        raise ValueError("simple_sa: NS = %d exceeds NFFT = %d" % (NS, NFFT))
    w = get_window(window, NS, fftbins=False)
    Sx = _psd_accum(x, w, NFFT, NS, NAVG)
    Sx /= float(NAVG)
    Sx /= float(NFFT ** 2)
    NFFTby2 = int(NFFT / 2)
    if x.dtype != 'complex128':
        f = fs * np.arange(NFFTby2) / float(NFFT)
        Sx = Sx[0:NFFTby2]
    else:
        f = fs * np.hstack((np.arange(-NFFTby2, 0), np.arange(NFFTby2))) / float(NFFT)
        Sx = np.hstack((Sx[NFFTby2:], Sx[0:NFFTby2]))
    return f, Sx


# ------------------------------------------------------------------------------------------------ the AWGN channel (sigsys.py:2335-2454)
def _awgn_input(x, name, ndim):
    x = _gpu_dtype(np.asarray(x))
    if x.ndim != ndim:
        raise ValueError("%s: a %d-D signal array" % (name, ndim))
    out = np.complex64 if x.dtype in (np.float32, np.complex64) else np.complex128
    return np.ascontiguousarray(x), np.dtype(out)


def _awgn_rows(x2d, out, mode, es_n0, ns, var_w, seed):
    """rows on the device: variance -> (g, sigma) -> y, each row with its own variance and its own stream"""
    nrow, n = x2d.shape
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n), dtype=out)
    seed = _ffi.new_seed() if seed is None else seed
    xd = _ffi.DeviceArray.from_host(x2d.reshape(-1))
    yd = _ffi.DeviceArray(nrow * n, out)
    gd, sd = _ffi.DeviceArray(nrow, np.float64), _ffi.DeviceArray(nrow, np.float64)
    try:
        _ffi.awgn_sigma_rows_dev(xd, n, nrow, mode, ns, es_n0, gd, sd, var_w_dB=var_w)
        _ffi.awgn_rows_dev(xd, yd, n, nrow, seed, gd=gd, sd=sd)
        return yd.to_host().reshape(nrow, n)
    finally:
        for d in (xd, yd, gd, sd):
            d.free()


def _awgn_rows_host(x2d, out, mode, es_n0, ns, var_w, seed):
    nrow, n = x2d.shape
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n), dtype=out)
    seed = _ffi.new_seed() if seed is None else seed
    wide = x2d.astype(np.complex128 if x2d.dtype.kind == "c" else np.float64)
    g, sigma = _ffi.awgn_sigma_host(np.var(wide, axis=1), mode, ns, es_n0, var_w)
    return _ffi.awgn_rows_host(x2d, g, sigma, seed, out)


def cpx_awgn(x, es_n0, ns, seed=None):
    """y = cpx_awgn(x, es_n0, ns), sigsys.py:2335-2370: x + sqrt(ns var(x) 10^(-es_n0 / 10) / 2) (randn + 1j randn), the variance, the draw
    and the sum on the GPU (csrc/symmap.hip's merge of partial moments, csrc/channel.hip: awgn_kernel).  x real or complex, one-dimensional.

    Deliberate differences (tests/golden/g23_conventions.json): the normals are this library's counter-based stream of `seed` (None: 64 bits
    of NumPy's global generator), not numpy.random.randn's values; float32 / complex64 in gives complex64 out (the float64 sum rounded once),
    everything else complex128; an empty x gives an empty array."""
    x, out = _awgn_input(x, "cpx_awgn", 1)
    return _awgn_rows(x[None, :], out, _ffi.SIGMA_AWGN, es_n0, ns, 0.0, seed)[0]


def cpx_awgn_host(x, es_n0, ns, seed=None):
    """cpx_awgn in NumPy (no GPU): the same stream, np.var and the reference's expressions -- the yardstick of cpx_awgn."""
    x, out = _awgn_input(x, "cpx_awgn", 1)
    return _awgn_rows_host(x[None, :], out, _ffi.SIGMA_AWGN, es_n0, ns, 0.0, seed)[0]


def cpx_awgn_rows(x2d, es_n0, ns, seed=None):
    """Beyond the reference: cpx_awgn of every row of a frame set in one pass -- row r has its own variance and the stream of row r."""
    x, out = _awgn_input(x2d, "cpx_awgn_rows", 2)
    return _awgn_rows(x, out, _ffi.SIGMA_AWGN, es_n0, ns, 0.0, seed)


def cpx_awgn2(x, es_n0, ns, var_w=0.0, seed=None):
    """y = cpx_awgn2(x, es_n0, ns, var_w), sigsys.py:2373-2454: the noise variance held at 10^(var_w / 10), the signal scaled by
    sqrt(1 / ns var_w / var(x) 10^(es_n0 / 10)).  Same kernels and the same deliberate differences as cpx_awgn."""
    x, out = _awgn_input(x, "cpx_awgn2", 1)
    return _awgn_rows(x[None, :], out, _ffi.SIGMA_AWGN2, es_n0, ns, var_w, seed)[0]


def cpx_awgn2_host(x, es_n0, ns, var_w=0.0, seed=None):
    """cpx_awgn2 in NumPy (no GPU): the yardstick of cpx_awgn2."""
    x, out = _awgn_input(x, "cpx_awgn2", 1)
    return _awgn_rows_host(x[None, :], out, _ffi.SIGMA_AWGN2, es_n0, ns, var_w, seed)[0]


# ------------------------------------------------------------------------------------------------ bit sources (sigsys.py:1947-2050)
# m_seq's feedback table: for register length m, the k in 1 ... m - 1 with taps[k] = 1 (its loop reads no other entry)
_MSEQ_TAPS = {2: (1,), 3: (2,), 4: (3,), 5: (3,), 6: (5,), 7: (4,), 8: (4, 5, 6), 9: (5,), 10: (7,), 11: (9,), 12: (6, 8, 11), 13: (9, 10, 12),
              14: (4, 8, 13), 15: (11,), 16: (2, 11, 15)}
_MSEQ_CACHE = {}
PN_HOST_MAX = 2 ** 16


def _mseq_bytes(m):
    """One period as uint8: an integer shift register started at all ones; out = the last cell, the new first cell = XOR over the taps k
    of (last cell ^ cell m - 1 - k), bit for bit the reference's double loop."""
    if m not in _MSEQ_TAPS:
        raise ValueError('Invalid length specified')
    if m not in _MSEQ_CACHE:
        taps, sr, mask = _MSEQ_TAPS[m], (1 << m) - 1, (1 << m) - 1      # bit j = cell j
        c = np.empty((1 << m) - 1, dtype=np.uint8)
        for n in range(c.size):
            last = (sr >> (m - 1)) & 1
            c[n] = last
            x = 0
            for k in taps:
                x ^= last ^ ((sr >> (m - 1 - k)) & 1)
            sr = ((sr << 1) | x) & mask
        _MSEQ_CACHE[m] = c
    return _MSEQ_CACHE[m]


def m_seq(m):
    """One period (2^m - 1 values 0. / 1., float64) of the m-sequence, m = 2 ... 16, sigsys.py:1983-2050 (host: an integer register)."""
    return _mseq_bytes(m).astype(np.float64)


def pn_rows(nrow, n, m=5, phases=None):
    """Beyond the reference: (nrow, n) uint8, row r = the m-sequence from phase phases[r] (default 0) (csrc/channel.hip: pn_kernel)."""
    c = _mseq_bytes(m)
    nrow, n = int(nrow), int(n)
    if nrow < 0 or n < 0:
        raise ValueError("pn_rows: negative size")
    ph = np.zeros(nrow, dtype=np.int64) if phases is None else np.ascontiguousarray(phases, dtype=np.int64).reshape(-1)
    if ph.size != nrow or np.any(ph < 0):
        raise ValueError("pn_rows: one non-negative phase per row")
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n), dtype=np.uint8)
    cd, pd, yd = _ffi.device_bytes_of(c), _ffi.device_bytes_of(ph), _ffi.DeviceBytes(nrow * n)
    try:
        _ffi.pn_rows_dev(cd, c.size, yd, n, nrow, phases_d=pd)
        return yd.read().reshape(nrow, n)
    finally:
        for d in (cd, pd, yd):
            d.free()


def pn_gen_host(n_bits, m=5):
    """pn_gen in NumPy (no GPU)."""
    return np.resize(m_seq(m), int(n_bits))


def pn_gen(n_bits, m=5):
    """n_bits values 0. / 1. (float64) of the m-sequence repeated, sigsys.py:1947-1980; past 2^16 values the period is tiled on the GPU."""
    if int(n_bits) <= PN_HOST_MAX:
        return pn_gen_host(n_bits, m)
    return pn_rows(1, n_bits, m)[0].astype(np.float64)


def random_bits_rows(nrow, n, seed=None):
    """Beyond the reference (its encoders draw np.random.randint on the host): (nrow, n) uint8 bits 0 / 1 of the counter-based bit stream of
    `seed`, row r = stream row r (csrc/channel.hip: randbits_kernel); _ffi.random_bits_host gives the same bits without a GPU."""
    nrow, n = int(nrow), int(n)
    if nrow < 0 or n < 0:
        raise ValueError("random_bits_rows: negative size")
    if nrow == 0 or n == 0:
        return np.zeros((nrow, n), dtype=np.uint8)
    seed = _ffi.new_seed() if seed is None else seed
    yd = _ffi.DeviceBytes(nrow * n)
    try:
        _ffi.random_bits_rows_dev(yd, n, nrow, seed)
        return yd.read().reshape(nrow, n)
    finally:
        yd.free()
