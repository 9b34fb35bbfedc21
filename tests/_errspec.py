"""The error spectrum of a transform-based FIR engine, measured against a host overlap-save in the engine's own precision.

max |y - ref| over the output's peak dilutes an error that sits in one twiddle entry, one bin of a taps spectrum or one output position of
a tile over the 8192 points of the tile, and low-pass taps leave most bins without signal.  This module holds what the two test files built
on it share (tests/test_errspec_cpu.py, tests/test_gpu_errspec.py); NumPy and SciPy only, nothing of the kernels.

Taps.    impulse_taps(P, F): P taps, zero but for one unit impulse in each polyphase branch r = 0 .. F - 1, at d_r = r (mod F), spread over the
         branch, b[P - 1] among them.  Every branch is a pure delay (magnitude 1 in every bin) and the expected output is a shifted copy of the
         input (exact_filter / exact_up / exact_dn / exact_updn): exact for float64 engines too.
         chirp_taps(P, F, cplx): the full-band linear-FM chirp exp(j pi (n - P/2)^2 / P) / sqrt(P) (its cosine for real signals) over F:
         dense taps with a smooth magnitude.  Their reference is the float64 oracle.
Input.   noise(n, dtype, seed): unit-variance Gaussian noise, complex samples over sqrt(2).
Yardstick.  yardstick(b, x, N, cdtype, L, M): overlap-save with N-point scipy.fft transforms in `cdtype` over the zero-stuffed signal, every
         M-th output kept.  A plain restatement: the tile size and the precision are the engine's, the split into passes is pocketfft's.
Statistics of e = y - ref, the first 8192 outputs (8192 L of .up) left out (measure()):
    R    ||e|| / ||ref||
    A    E_k = the mean of |FFT_8192(e)|^2 over the S >= 64 whole segments of 8192 samples; A = max_k E_k / m_k, m_k the circular running
         median of E over 129 bins.  No window: every tile size divides 8192, so a fault of one bin falls on the grid.  For .up the worst of
         e and of each output phase e[r::L].
    B    |e|^2 averaged per position of the engine's output period V (output j at position (j step) mod V: step = M for a decimator whose
         tiles are tiles of the input); B = max / median over the positions that occur.

two_pass_model() is a float32 model of the 8192-point tile, 64 x 128 with one inter-pass twiddle table per direction, whose tables and taps
spectrum a test can damage (tests/test_errspec_cpu.py shows what today's metric lets through and A and B do not)."""
import functools

import numpy as np
import scipy.fft
import scipy.ndimage

SEG = 8192       # segment of the error spectrum; every tile size (8192, 4096, 2048) divides it
MEDIAN_BINS = 129
MIN_SEGMENTS = 64


# ------------------------------------------------------------------------------------------------ input and taps
@functools.lru_cache(maxsize=4)
def _noise(n, name, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(name)
    if dt.kind == "c":
        x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(dt)
    else:
        x = rng.standard_normal(n).astype(dt)
    x.setflags(write=False)
    return x


def noise(n, dtype, seed):
    """Unit-variance Gaussian noise (read-only: one array per (n, dtype, seed) is shared among the cases)."""
    return _noise(int(n), np.dtype(dtype).name, int(seed))


def impulse_positions(P, F):
    """d_r, r = 0 .. F - 1: d_r = r (mod F), d_r < P, spread over the taps of branch r; the branch of tap P - 1 has its impulse there."""
    P, F = int(P), int(F)
    if not 1 <= F <= P:
        raise ValueError("impulse_positions: 1 <= F <= P")
    d = np.empty(F, np.int64)
    for r in range(F):
        T = (P - r + F - 1) // F                     # taps of branch r: r, r + F, ..., r + (T - 1) F
        d[r] = r + F * (((2 * r + 1) * T) // (2 * F))
    d[(P - 1) % F] = P - 1
    assert np.all(d % F == np.arange(F)) and np.all(d < P) and np.all(d >= 0)
    return d


def impulse_taps(P, F=1):
    """(b, d): float64 taps of P zeros with b[d_r] = 1."""
    d = impulse_positions(P, F)
    b = np.zeros(int(P))
    b[d] = 1.0
    return b, d


def chirp_taps(P, F=1, cplx=True):
    """The full-band chirp over F (as the low-pass designs of the other tests scale with 1 / F); complex128, or its cosine in float64."""
    n = np.arange(int(P), dtype=np.float64)
    ph = np.pi * (n - P / 2.0) ** 2 / P
    return (np.exp(1j * ph) if cplx else np.cos(ph)) / np.sqrt(P) / F


def tone_perturbation(P, k0, delta, cplx=True):
    """delta exp(2 pi j k0 n / 8192) / P over the P taps (complex; twice its cosine for real signals): the SEG-point taps spectrum rises by
    delta at bin k0 (and at -k0 for the cosine), inside a main lobe of SEG / P bins to either side."""
    ph = 2.0 * np.pi * ((int(k0) * np.arange(int(P), dtype=np.int64)) % SEG) / SEG
    return delta * (np.exp(1j * ph) if cplx else 2.0 * np.cos(ph)) / P


# ------------------------------------------------------------------------------------------------ the exact references of impulse taps
def _wide(x):
    """The type the exact sums are taken in: float64 inputs in long double, float32 inputs in float64 (a sum of M of them is exact)."""
    x = np.asarray(x)
    if x.dtype in (np.float64, np.complex128):
        return x.astype(np.clongdouble if x.dtype.kind == "c" else np.longdouble)
    return x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)


def _with_past(x, hist, lead):
    """`lead` samples in front of x[0]: zeros, the last of them the history."""
    x = _wide(x)
    past = np.zeros(lead, x.dtype)
    if hist is not None and len(hist):
        h = _wide(hist).astype(x.dtype)
        past[lead - len(h):] = h
    return np.concatenate([past, x])


def exact_filter(d, x, hist=None):
    """y[n] = x[n - d_0]."""
    d0, n = int(np.asarray(d).reshape(-1)[0]), len(x)
    return _with_past(x, hist, d0)[:n]


def exact_up(d, x, L, hist=None):
    """y[i L + r] = L x[i - (d_r - r) / L]."""
    d, n = np.asarray(d), len(x)
    assert len(d) == L
    t = (d - np.arange(L)) // L
    lead = int(t.max())
    xp = _with_past(x, hist, lead)
    y = np.empty((n, L), xp.dtype)
    for r in range(L):
        y[:, r] = L * xp[lead - t[r]:lead - t[r] + n]
    return y.reshape(-1)


def exact_dn(d, x, M, hist=None):
    """y[i] = sum_r x[i M - d_r], i < floor(n / M)."""
    d, n = np.asarray(d), len(x)
    assert len(d) == M
    lead = int(d.max())
    xp = _with_past(x, hist, lead)
    cnt = n // M
    y = np.zeros(cnt, xp.dtype)
    for r in range(M):
        s = lead - int(d[r])
        y += xp[s:s + cnt * M:M][:cnt]
    return y


def exact_updn(d, x, L, M):
    """Every M-th sample of the .up result."""
    y = exact_up(d, x, L)
    return y[::M][:(len(x) * L) // M].copy()


# ------------------------------------------------------------------------------------------------ the yardstick
def ols_host(b, x, N, cdtype=np.complex64, overlap=None, H=None):
    """lfilter(b, 1, x) by overlap-save: N-point scipy.fft transforms of `cdtype` tiles, overlap len(b) - 1 unless given, the taps spectrum
    from float64 and rounded once.  Complex result."""
    cdtype = np.dtype(cdtype)
    P, n = len(b), len(x)
    ov = P - 1 if overlap is None else int(overlap)
    V = N - ov
    assert ov >= P - 1 and V > 0
    if H is None:
        H = scipy.fft.fft(np.asarray(b, np.complex128), N).astype(cdtype)
    ntiles = -(-n // V)
    xp = np.zeros(ov + ntiles * V, cdtype)
    xp[ov:ov + n] = x
    out = np.empty(ntiles * V, cdtype)
    step = max(1, (1 << 22) // N)                    # tiles per batch
    for t0 in range(0, ntiles, step):
        t1 = min(ntiles, t0 + step)
        tiles = np.lib.stride_tricks.as_strided(xp[t0 * V:], shape=(t1 - t0, N), strides=(V * xp.itemsize, xp.itemsize))
        Y = scipy.fft.ifft(scipy.fft.fft(tiles, axis=1) * H, axis=1)
        assert Y.dtype == cdtype, Y.dtype            # scipy.fft keeps single precision (numpy.fft before 2.0 does not)
        out[t0 * V:t1 * V] = Y[:, ov:].reshape(-1)
    return out[:n]


def yardstick(b, x, N, cdtype=np.complex64, L=1, M=1, overlap=None):
    """.filter / .up / .dn / .updn of the yardstick: the filter over the zero-stuffed signal times L, every M-th output kept; real when the
    signal and the taps are."""
    x = np.asarray(x)
    if L > 1:
        u = np.zeros(len(x) * L, x.dtype)
        u[::L] = x * x.dtype.type(L)
    else:
        u = x
    y = ols_host(b, u, N, cdtype, overlap)
    if M > 1:
        y = y[::M][:len(u) // M]
    if x.dtype.kind != "c" and not np.iscomplexobj(b):
        y = y.real
    return np.ascontiguousarray(y)


def tile_overlap(taps_per_phase, block, N):
    """(overlap, V) of a tile engine: taps per phase - 1 rounded up to whole blocks, at least one (csrc/ols_tables.hpp)."""
    ov = max(block, -(-(taps_per_phase - 1) // block) * block)
    return ov, N - ov


# ------------------------------------------------------------------------------------------------ statistics
def error_of(y, ref):
    """y - ref in float64 / complex128 (the difference itself in ref's type, which is long double for float64 engines)."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    wide = np.result_type(y.dtype, ref.dtype)
    e = y.astype(wide) - ref.astype(wide)
    return e.astype(np.complex128 if e.dtype.kind == "c" else np.float64)


def spectrum_stat(e):
    """(A, worst bin, E): E_k over the whole segments of SEG samples, against its circular running median."""
    S = len(e) // SEG
    assert S >= MIN_SEGMENTS, (len(e), S)
    E = np.mean(np.abs(scipy.fft.fft(e[:S * SEG].reshape(S, SEG), axis=1)) ** 2, axis=0)
    m = scipy.ndimage.median_filter(E, size=MEDIAN_BINS, mode="wrap")
    ratio = E / np.where(m > 0, m, np.inf) if np.any(m > 0) else np.zeros_like(E)
    k = int(np.argmax(ratio))
    return float(ratio[k]), k, E


def position_stat(e, first, period, step=1):
    """(B, worst position): |e|^2 averaged per position ((first + j) step) mod period."""
    pos = ((first + np.arange(len(e), dtype=np.int64)) * step) % period
    cnt = np.bincount(pos, minlength=period)
    pw = np.bincount(pos, weights=np.abs(e) ** 2, minlength=period)
    hit = cnt > 0
    mean = pw[hit] / cnt[hit]
    med = float(np.median(mean))
    if med <= 0:
        return (0.0 if float(mean.max()) == 0 else float("inf")), int(np.flatnonzero(hit)[np.argmax(mean)])
    return float(mean.max() / med), int(np.flatnonzero(hit)[np.argmax(mean)])


def measure(y, ref, L=1, period=None, step=1):
    """R, A (with its bin and the phase it was found in: -1 = all outputs; A_each / bin_each: of all outputs and of every phase) and B (with
    its position; None without a period) of e = y - ref behind the first SEG * L outputs."""
    skip = SEG * L
    e = error_of(y, ref)[skip:]
    r = np.asarray(ref)[skip:]
    out = {"R": float(np.linalg.norm(e) / float(np.linalg.norm(r.astype(np.complex128 if r.dtype.kind == "c" else np.float64))))}
    A, k, _ = spectrum_stat(e)
    out.update(A=A, bin=k, phase=-1, A_each=[A], bin_each=[k])   # A_each: all outputs, then phase 0 .. L - 1
    if L > 1:
        for ph in range(L):
            a, k, _ = spectrum_stat(e[ph::L])
            out["A_each"].append(a)
            out["bin_each"].append(k)
            if a > out["A"]:
                out.update(A=a, bin=k, phase=ph)
    if period is not None:
        out["B"], out["pos"] = position_stat(e, skip, period, step)
    else:
        out["B"], out["pos"] = None, None
    return out


def peak_err(y, ref):
    """Today's metric: max |y - ref| over the peak of ref."""
    return float(np.max(np.abs(error_of(y, ref))) / np.max(np.abs(np.asarray(ref).astype(np.complex128))))


# ------------------------------------------------------------------------------------------------ a float32 model of the 8192-point tile
N1, N2 = 64, 128


def two_pass_tables():
    """(forward, inverse) inter-pass twiddles T[k1, n2] = exp(-/+ 2 pi j k1 n2 / 8192) in complex64, from float64."""
    ph = 2.0 * np.pi * np.outer(np.arange(N1), np.arange(N2)) / (N1 * N2)
    return np.exp(-1j * ph).astype(np.complex64), np.exp(1j * ph).astype(np.complex64)


def two_pass_fft(x, T):
    """8192-point DFTs of the rows of x: n = 128 n1 + n2, k = k1 + 64 k2; 64-point transforms over n1, T, 128-point transforms over n2."""
    a = scipy.fft.fft(x.reshape(-1, N1, N2), axis=1) * T
    X = scipy.fft.fft(a, axis=2)
    return X.transpose(0, 2, 1).reshape(-1, N1 * N2)


def two_pass_ifft(X, T):
    """The mirrored inverse: 128-point inverse transforms over k2, T (the conjugate table), 64-point inverse transforms over k1."""
    a = scipy.fft.ifft(X.reshape(-1, N2, N1).transpose(0, 2, 1), axis=2) * T
    return scipy.fft.ifft(a, axis=1).reshape(-1, N1 * N2)


def two_pass_model(b, x, fwd=None, inv=None, H=None):
    """Overlap-save of complex64 x through the model tile; overlap len(b) - 1 rounded up to 512 as the 8192-point engine has it.  `fwd`,
    `inv` and `H` replace the clean tables (two_pass_tables(), model_H(b))."""
    N = N1 * N2
    clean_f, clean_i = two_pass_tables()
    fwd = clean_f if fwd is None else fwd
    inv = clean_i if inv is None else inv
    H = model_H(b) if H is None else H
    ov, V = tile_overlap(len(b), 512, N)
    n = len(x)
    ntiles = -(-n // V)
    xp = np.zeros(ov + ntiles * V, np.complex64)
    xp[ov:ov + n] = x
    tiles = np.lib.stride_tricks.as_strided(xp, shape=(ntiles, N), strides=(V * xp.itemsize, xp.itemsize))
    Y = two_pass_ifft(two_pass_fft(np.ascontiguousarray(tiles), fwd) * H, inv)
    assert Y.dtype == np.complex64, Y.dtype
    return Y[:, ov:].reshape(-1)[:n]


def model_H(b):
    return scipy.fft.fft(np.asarray(b, np.complex128), N1 * N2).astype(np.complex64)
