"""Synchronization on the GPU: the non-data-aided symbol timing loop, the decision-directed carrier phase tracking loop of
sk_dsp_comm.synchronization and the two impairment helpers that exercise them (synchronization.py:43-313 of the reference), over frame sets
(csrc/timing.hip; csrc/carrier.hip).

    NDA_symb_sync(z, Ns, L, BnTs, zeta=0.707, I_ord=3)                                      the reference's call: one row of the kernel
    NDA_symb_sync_rows(z2d, ...)                                                            beyond the reference: every row a frame from rest

    DD_carrier_sync(z, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False)      the reference's call: one row of the kernel
    DD_carrier_sync_rows(z2d, ...)                                                          beyond the reference: every row a frame from rest
    phase_step(z, ns, p_step, n_step), time_step(z, ns, t_step, n_step)                     the reference's calls
    phase_step_rows(z2d, ...), time_step_rows(z2d, ...)                                     over rows, the step a scalar or one value per row
and a *_host form of each in NumPy (no GPU) that performs the kernel's operations one by one and gives the same bits.

Kept from the reference: np.sign(0) = 0, so a decision can be 0 (type 2 then divides by it as NumPy's complex division does); theta_h is logged
behind the wrap and open_loop zeroes theta_hat after logging; MQAM frames are scaled by np.std(z) sqrt(3 / (2 (M - 1))) and z_prime is multiplied back;
MQAM M = 2 decides with x_m = 1.

Deliberate differences (tests/golden/g27_conventions.json):
  * MPSK above 4: the reference calls .astype(np.int), which NumPy >= 1.24 no longer has (AttributeError); here the documented intent,
    mod(rint(angle M / 2 / pi), M), with M up to 32.
  * an unsupported M, mod_type or type raises ValueError where the reference prints a message and returns zeros.
  * z must be complex (the reference fails on a real array when it stores into zeros_like(z)): TypeError.
  * complex64 is a storage type: samples are widened at the load, the loop runs in float64, z_prime / a_hat are rounded once at the store and e_phi /
    theta_h are float64.  (The reference rounds z_prime to float32 inside the loop and goes on in mixed scalar types; that is not reproduced.)
  * the angle functions are the project's own (sincos to 2 ulp, atan2 rounded to nearest), so that host and device agree to the bit; against the
    reference's libm the outputs differ by the rounding noise the loop carries (tests/test_carrier_cpu.py bounds it by the reference's own).
  * the MQAM scale is the deterministic moment merge of qam_gray_decode_rows; z / z_scale is the product with r = 1 / z_scale per component (as NumPy
    divides a complex array by a real scalar) and z_prime is multiplied back by 1 / r: one rounding from the reference's z_scale.
  * phase_step / time_step of a complex64 signal return complex64 (the reference widens to complex128); negative steps are refused.

NDA_symb_sync keeps the reference's conventions (tests/golden/g28_conventions.json): the zero sample in front, its loop range, zz[0] = e_tau[0] = 0, the
last stored symbol dropped, epsilon held while the loop coasts, zz /= np.std(zz) over the trimmed output (one output: 0 / 0 = nan).  It differs in this:
  * |z|^2 in the detector is re re + im im (the reference squares hypot); the angle is the project's atan2, rounded to nearest.
  * Ns outside 2 ... 16, L outside 0 ... 8 or I_ord outside 1, 2, 3 raise ValueError (the reference logs and fails on an unbound name).
  * Ns = 2 with I_ord >= 2 and an odd len(z) >= 3 raises ValueError: there the reference's slices run past its array when the counter underflows on the
    last sample, and it raises; here the length alone decides.
  * complex64 is storage, as above; a real z is widened exactly.
  * the rows' np.std is np.std's two passes with sums in a fixed order (within 3e-15 of np.std, relative, for rows up to 8192 symbols).
"""
import numpy as np

from . import _ffi

__all__ = ["NDA_symb_sync", "NDA_symb_sync_host", "NDA_symb_sync_rows", "NDA_symb_sync_rows_host", "DD_carrier_sync", "DD_carrier_sync_host", "DD_carrier_sync_rows", "DD_carrier_sync_rows_host", "phase_step", "phase_step_host", "phase_step_rows",
           "phase_step_rows_host", "time_step", "time_step_host", "time_step_rows", "time_step_rows_host"]

_OUTPUTS = _ffi.CAR_OUTPUTS


def _one_row(z, name):
    z = np.asarray(z)
    if z.ndim != 1:
        raise ValueError("%s: z must be one-dimensional (got shape %r)" % (name, z.shape))
    if z.dtype not in (np.complex64, np.complex128):
        raise TypeError("%s: z must be complex64 or complex128 (got %s)" % (name, z.dtype))
    return z.reshape(1, -1)


def _one_row_nda(z):
    z = np.asarray(z)
    if z.ndim != 1:
        raise ValueError("NDA_symb_sync: z must be one-dimensional (got shape %r)" % (z.shape,))
    return z.reshape(1, -1)


def NDA_symb_sync_rows(z2d, Ns, L, BnTs, zeta=0.707, I_ord=3, start=0, normalize=True, max_symbols=None, outputs=_ffi.NDA_OUTPUTS):
    """Beyond the reference: NDA_symb_sync of every row's z2d[row, start:] in one launch, every row a frame from rest.  BnTs: a scalar, or one value per
    row.  Returns the selected of zz (z2d's complex dtype) and e_tau (float64), nrow x cap each and zero behind counts[row], then counts (int64): the
    reference's output length per row.  cap is the number of loop iterations, an exact upper bound, or max_symbols where that is lower; a row that
    produces more raises ValueError (the kernel keeps counting and stops storing).  normalize=False returns the raw interpolants, for a caller whose
    next stage scales by itself (DD_carrier_sync_rows for MQAM does).  One lane of the GPU per row (csrc/timing.hip)."""
    return _ffi.nda_rows(z2d, Ns, L, BnTs, zeta, I_ord, start, normalize, max_symbols, outputs)


def NDA_symb_sync_rows_host(z2d, Ns, L, BnTs, zeta=0.707, I_ord=3, start=0, normalize=True, max_symbols=None, outputs=_ffi.NDA_OUTPUTS):
    """NDA_symb_sync_rows in NumPy (no GPU): the kernel's operations one by one, vectorised over rows, with the device's bits"""
    return _ffi.nda_rows_host(z2d, Ns, L, BnTs, zeta, I_ord, start, normalize, max_symbols, outputs)


def _trim(res):
    zz, e_tau, counts = res
    return zz[0, :counts[0]], e_tau[0, :counts[0]]


def NDA_symb_sync(z, Ns, L, BnTs, zeta=0.707, I_ord=3):
    """zz, e_tau = NDA_symb_sync(z, Ns, L, BnTs, zeta=0.707, I_ord=3), synchronization.py:43-166: non-data-aided symbol timing recovery of a complex
    baseband signal at nominally Ns samples per symbol.  L: the timing error detector is smoothed over 2L + 1 symbols; BnTs: loop bandwidth times symbol
    period; I_ord: the Farrow interpolator's order, 1, 2 or 3.  zz: the interpolants at the symbol rate, scaled to unit standard deviation; e_tau: the
    timing error.  One row of the kernel behind NDA_symb_sync_rows; the module docstring lists what is kept and what differs."""
    return _trim(NDA_symb_sync_rows(_one_row_nda(z), Ns, L, BnTs, zeta, I_ord))


def NDA_symb_sync_host(z, Ns, L, BnTs, zeta=0.707, I_ord=3):
    """NDA_symb_sync in NumPy (no GPU): one row of NDA_symb_sync_rows_host"""
    return _trim(NDA_symb_sync_rows_host(_one_row_nda(z), Ns, L, BnTs, zeta, I_ord))


def DD_carrier_sync_rows(z2d, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False, start=0, step=1, outputs=_OUTPUTS):
    """Beyond the reference: DD_carrier_sync of every row's z2d[row, start::step] in one launch, every row a frame from rest (theta_hat = 0, vi = 0).
    BnTs: a scalar, or one value per row (a sweep of loop bandwidths).  outputs: which of ('z_prime', 'a_hat', 'e_phi', 'theta_h') to produce, in
    that order of the returned tuple; only those cost memory traffic (a BER loop needs 'z_prime' alone).  z_prime / a_hat have z2d's dtype
    (complex64 / complex128), e_phi / theta_h are float64.  One lane of the GPU per row (csrc/carrier.hip)."""
    return _ffi.dd_carrier_rows(z2d, _ffi.carrier_family(mod_type), M, BnTs, zeta, type, open_loop, start, step, outputs)


def DD_carrier_sync_rows_host(z2d, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False, start=0, step=1, outputs=_OUTPUTS, r=None):
    """DD_carrier_sync_rows in NumPy (no GPU): the kernel's operations one by one, vectorised over rows and sequential over symbols.  r: the MQAM
    rows' 1 / z_scale; default NumPy's own np.std (within the merge's accuracy of the device's), pass _ffi.qam_scale_rows' for the device's bits."""
    return _ffi.dd_carrier_rows_host(z2d, _ffi.carrier_family(mod_type), M, BnTs, zeta, type, open_loop, start, step, outputs, r)


def DD_carrier_sync(z, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False):
    """z_prime, a_hat, e_phi, theta_h = DD_carrier_sync(z, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False), synchronization.py:169-275:
    decision-directed carrier phase tracking of a complex baseband signal at one sample per symbol.  M: the order (MPSK 2, 4, 8, 16, 32; MQAM 2, 4, 16,
    64, 256); BnTs: loop bandwidth times symbol period; type: the phase detector (0 ML, 1 heuristic, 2 Ouyang and Wang).  One row of the kernel
    behind DD_carrier_sync_rows; the module docstring lists what is kept and what differs."""
    return tuple(v[0] for v in DD_carrier_sync_rows(_one_row(z, "DD_carrier_sync"), M, BnTs, zeta, mod_type, type, open_loop))


def DD_carrier_sync_host(z, M, BnTs, zeta=0.707, mod_type='MPSK', type=0, open_loop=False):
    """DD_carrier_sync in NumPy (no GPU): one row of DD_carrier_sync_rows_host"""
    return tuple(v[0] for v in DD_carrier_sync_rows_host(_one_row(z, "DD_carrier_sync"), M, BnTs, zeta, mod_type, type, open_loop))


# ---- phase_step / time_step -------------------------------------------------------------------------------------------------------------
def _imp_rows(z2d, ns, n_step, name):
    z = np.asarray(z2d)
    if z.ndim != 2:
        raise ValueError("%s: a 2-D array, one frame per row" % name)
    if z.dtype not in (np.complex64, np.complex128):
        raise TypeError("%s: z must be complex64 or complex128 (got %s)" % (name, z.dtype))
    if int(ns) != ns or ns < 1 or int(n_step) != n_step or n_step < 0:
        raise ValueError("%s: ns must be a positive integer and n_step a non-negative one" % name)
    return np.ascontiguousarray(z), int(ns), int(n_step)


def _per_row(v, nrow, name):
    v = np.asarray(v)
    if v.ndim == 0:
        return None
    if v.shape != (nrow,):
        raise ValueError("%s: a scalar, or one value per row" % name)
    return v


def _phase_factors(p_step, nrow):
    """np.exp(1j theta) of the reference, for the scalar or per row"""
    per = _per_row(p_step, nrow, "p_step")
    if per is None:
        return complex(np.exp(1j * np.array([float(p_step)]))[0]), None
    f = np.exp(1j * per.astype(np.float64))
    return 1.0 + 0j, np.ascontiguousarray(np.stack([f.real, f.imag], axis=1))


def phase_step_rows_host(z2d, ns, p_step, n_step):
    """phase_step_rows in NumPy (no GPU): every ns-th sample times 1 + 0j in front of symbol n_step and np.exp(1j p_step) from there on, the complex
    product written out: re = a c - b d, im = a d + b c in float64, one rounding to z2d's dtype"""
    z, ns, n_step = _imp_rows(z2d, ns, n_step, "phase_step_rows")
    f, per = _phase_factors(p_step, z.shape[0])
    zs = z[:, ::ns].astype(np.complex128)
    c, d = np.ones(zs.shape), np.zeros(zs.shape)
    c[:, n_step:], d[:, n_step:] = (f.real, f.imag) if per is None else (per[:, :1], per[:, 1:])
    out = np.empty(zs.shape, dtype=np.complex128)
    out.real, out.imag = zs.real * c - zs.imag * d, zs.real * d + zs.imag * c
    return out.astype(z.dtype)


def _time_lens(n, ns, t_step, n_step, nrow):
    per = _per_row(t_step, nrow, "t_step")
    steps = np.full(nrow, int(t_step), dtype=np.int64) if per is None else per.astype(np.int64)
    if (per is not None and np.any(per != steps)) or (per is None and int(t_step) != t_step) or np.any(steps < 0):
        raise ValueError("time_step_rows: t_step must be a non-negative integer")
    lens = {_ffi.time_step_len(n, ns, int(t), n_step) for t in steps} if nrow else {n}
    if len(lens) != 1:
        raise ValueError("time_step_rows: these t_step values give rows of different lengths (the step runs past the end of the waveform)")
    return per, steps, lens.pop()


def time_step_rows_host(z2d, ns, t_step, n_step):
    """time_step_rows in NumPy (no GPU): index arithmetic only"""
    z, ns, n_step = _imp_rows(z2d, ns, n_step, "time_step_rows")
    nrow, n = z.shape
    _, steps, n_out = _time_lens(n, ns, t_step, n_step, nrow)
    out = np.zeros((nrow, n_out), dtype=z.dtype)
    edge = min(n, ns * n_step)
    for r in range(nrow):
        out[r, :edge] = z[r, :edge]
        rest = z[r, ns * n_step + int(steps[r]):]
        out[r, edge:edge + rest.size] = rest
    return out


def phase_step_rows(z2d, ns, p_step, n_step):
    """Beyond the reference: phase_step of every row in one launch; p_step a scalar or one value per row (csrc/carrier.hip: impair_rows_kernel).
    Exact against the reference: the rotation is its complex product with host-computed (cos, sin), no fused multiply-add."""
    z, ns, n_step = _imp_rows(z2d, ns, n_step, "phase_step_rows")
    nrow, n = z.shape
    f, per = _phase_factors(p_step, nrow)
    n_out = -(-n // ns)
    if nrow == 0 or n_out == 0:
        return np.zeros((nrow, n_out), dtype=z.dtype)
    xd, yd = _ffi.DeviceArray.from_host(z.reshape(-1)), _ffi.DeviceArray(nrow * n_out, z.dtype)
    fd = None if per is None else _ffi.DeviceArray.from_host(per.reshape(-1))
    try:
        _ffi.phase_step_rows_dev(xd, yd, n, nrow, ns, n_step, f, fd)
        return yd.to_host().reshape(nrow, n_out)
    finally:
        for d in (xd, yd, fd):
            if d is not None:
                d.free()


def time_step_rows(z2d, ns, t_step, n_step):
    """Beyond the reference: time_step of every row in one launch; t_step a scalar or one value per row (which must give rows of one length).
    Exact: a gather with zero fill."""
    z, ns, n_step = _imp_rows(z2d, ns, n_step, "time_step_rows")
    nrow, n = z.shape
    per, steps, n_out = _time_lens(n, ns, t_step, n_step, nrow)
    if nrow == 0 or n_out == 0:
        return np.zeros((nrow, n_out), dtype=z.dtype)
    xd, yd = _ffi.DeviceArray.from_host(z.reshape(-1)), _ffi.DeviceArray(nrow * n_out, z.dtype)
    td = None if per is None else _ffi.device_bytes_of(steps)
    try:
        _ffi.time_step_rows_dev(xd, yd, n, nrow, ns, n_step, int(steps[0]), td, n_out)
        return yd.to_host().reshape(nrow, n_out)
    finally:
        for d in (xd, yd, td):
            if d is not None:
                d.free()


def phase_step(z, ns, p_step, n_step):
    """z_rot = phase_step(z, ns, p_step, n_step), synchronization.py:295-313: z[::ns] with a phase step of p_step radians from symbol n_step on"""
    return phase_step_rows(_one_row(z, "phase_step"), ns, p_step, n_step)[0]


def phase_step_host(z, ns, p_step, n_step):
    return phase_step_rows_host(_one_row(z, "phase_step"), ns, p_step, n_step)[0]


def time_step(z, ns, t_step, n_step):
    """z_step = time_step(z, ns, t_step, n_step), synchronization.py:278-292: t_step samples removed at sample ns n_step, t_step zeros appended"""
    return time_step_rows(_one_row(z, "time_step"), ns, t_step, n_step)[0]


def time_step_host(z, ns, t_step, n_step):
    return time_step_rows_host(_one_row(z, "time_step"), ns, t_step, n_step)[0]
