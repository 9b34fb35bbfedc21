"""The Welch primitive on the MI355X (csrc/psd.hip) and sigsys.psd / my_psd / simple_sa on top of it: the captured
reference (g16), full-size workloads against the host float64 restatement (sigsys.psd_accum_host), coherent inputs,
non-finite samples, determinism, the device entry point's footprint and the engine record.

Tolerances for float32 / complex64 signals:
  (a) max |S - S_ref| <= 1e-6 max S_ref                                   (the project's float32 contract)
  (b) on bins >= 1e-5 of the peak, max |S - S_ref| / S_ref <= max(8 y, 1e-7), y being the same figure of a NumPy complex64
      restatement (np.fft on complex64 segments, float32 window) of the same input -- computed here, never from the kernel.
float64 / complex128: (a) with 1e-12."""
import numpy as np
import pytest
from scipy.signal import get_window, windows

from sk_dsp_comm_amd import _ffi, config, sigsys as ss
from test_psd_cpu import g16_cases, g16_input, g16_call, peak_err

pytestmark = pytest.mark.gpu


class _cfg:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: getattr(config, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(config, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(config, k, v)
        return False


def yardstick_c64(x, window, n_fft, step, nseg):
    """The primitive in NumPy single precision: float32 window, complex64 (float32) segments, np.fft in complex64, |X|^2 and the
    segment sum in float64."""
    w = np.asarray(window, dtype=np.float32)
    xs = np.ascontiguousarray(x, dtype=np.complex64 if np.iscomplexobj(x) else np.float32)
    S = np.zeros(n_fft)
    it = xs.itemsize
    blk = max(1, (1 << 21) // n_fft)
    for i0 in range(0, nseg, blk):
        k = min(blk, nseg - i0)
        seg = np.lib.stride_tricks.as_strided(xs[i0 * step:], shape=(k, w.size), strides=(step * it, it), writeable=False)
        X = np.fft.fft(seg * w, n_fft, axis=1)
        assert X.dtype == np.complex64
        S += (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2).sum(axis=0)
    return S


def bin_err(S, ref):
    m = ref >= 1e-5 * ref.max()
    return float(np.max(np.abs(S[m] - ref[m]) / ref[m]))


def check_primitive(x, window, n_fft, step, nseg, label):
    """Runs the kernel on host vector x and holds it to (a) and (b) (or to 1e-12 for float64 / complex128)."""
    _ffi.debug_path()
    S = _ffi.psd_accum(x, window, n_fft, step, nseg)
    assert "psd" in _ffi.debug_path()
    assert S.shape == (n_fft,) and S.dtype == np.float64
    ref = ss.psd_accum_host(x, window, n_fft, step, nseg)
    ea = peak_err(S, ref)
    if x.dtype in (np.float64, np.complex128):
        print("%s: peak-relative %.2e" % (label, ea))
        assert ea <= 1e-12, (label, ea)
        return S
    eb = bin_err(S, ref)
    y = bin_err(yardstick_c64(x, window, n_fft, step, nseg), ref)
    print("%s: peak-relative %.2e, per-bin %.2e (yardstick %.2e, bound %.2e)" % (label, ea, eb, y, max(8 * y, 1e-7)))
    assert ea <= 1e-6, (label, ea)
    assert eb <= max(8 * y, 1e-7), (label, eb, y)
    return S


def _noise(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n, dtype=np.float32 if dtype in (np.float32, np.complex64) else np.float64)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(n, dtype=x.dtype)
    return x.astype(dtype, copy=False)


def _welch(n, n_fft, overlap):
    step, K = ss._psd_segments(n, n_fft, overlap)
    return step, K


def test_g16_through_gpu():
    g, cases = g16_cases()
    _ffi.debug_path()
    for c in cases:
        x, ref = g16_input(g, c), g[c["key"]]
        P, f = g16_call(c, x)
        assert P.shape == ref.shape and P.dtype == np.float64 and np.allclose(f, g[c["key"] + "_f"], rtol=1e-15, atol=0), c
        if np.all(np.isnan(ref)):
            assert np.all(np.isnan(P)), c
            continue
        n_fft = c["args"].get("n_fft", c["args"].get("NFFT"))
        narrow = x.dtype in (np.float32, np.complex64) and ss._psd_served(n_fft)
        e = peak_err(P, ref)
        assert e <= (1e-6 if narrow else 1e-12), (c, e)
        if narrow:
            with _cfg(precision="double"):
                Pd, _ = g16_call(c, x)
            assert peak_err(Pd, ref) <= 1e-12, c
            if c["fn"] == "psd":
                step, K = _welch(c["Q"], n_fft, c["args"]["overlap_percent"])
                check_primitive(x, windows.hann(n_fft), n_fft, step, K, "g16 %s" % c["key"])
        elif x.dtype in (np.float64, np.complex128) and ss._psd_served(n_fft):
            with _cfg(precision="single"):
                Ps, _ = g16_call(c, x)
            assert peak_err(Ps, ref) <= 1e-6, c
    assert "psd" in _ffi.debug_path()


@pytest.mark.parametrize("dtype", [np.complex64, np.float32])
def test_full_size_2p26(dtype):
    n, n_fft = 1 << 26, 1024
    x = _noise(n, dtype, 26)
    step, K = _welch(n, n_fft, 50)
    assert K == 131070
    check_primitive(x, windows.hann(n_fft), n_fft, step, K, "2^26 %s" % np.dtype(dtype).name)
    # and through the public function: noise of unit variance per component reads its variance
    Px, f = ss.psd(x, n_fft)
    assert Px.shape == ((n_fft,) if dtype == np.complex64 else (n_fft // 2 + 1,))
    assert abs(np.mean(Px[1:-1]) / (2.0 if dtype == np.complex64 else 1.0) - 1.0) < 0.01


@pytest.mark.parametrize("n_fft,dtype,overlap,ns", [
    (64, np.complex64, 50, None), (128, np.complex64, 50, None), (256, np.complex64, 50, None), (512, np.complex64, 50, None),
    (2048, np.complex64, 50, None), (4096, np.complex64, 50, None),
    (64, np.float32, 50, None), (4096, np.float32, 50, None),
    (1024, np.float32, 37, None),      # odd hop: 645 samples, pairs of segments an odd distance apart
    (256, np.complex64, 37, None),
    (1024, np.complex64, 75, None),
    (1024, np.complex64, 50, 1000),    # ns < n_fft
    (512, np.float32, 0, 300),
])
def test_2p24_shapes(n_fft, dtype, overlap, ns):
    n = 1 << 24
    x = _noise(n, dtype, n_fft + overlap)
    if ns is None:
        step, K = _welch(n, n_fft, overlap)
        w = get_window("hann", n_fft)
    else:
        step = ns - int(round(overlap / 100 * ns))
        K = (n - ns) // step + 1
        w = get_window("hann", ns, fftbins=False)
    check_primitive(x, w, n_fft, step, K, "2^24 n_fft %d %s overlap %d ns %s" % (n_fft, np.dtype(dtype).name, overlap, ns))


@pytest.mark.parametrize("dtype,n_fft", [(np.float64, 1024), (np.complex128, 1024), (np.complex128, 4096), (np.float64, 4096),
                                         (np.complex128, 64), (np.float64, 128)])
def test_float64_shapes(dtype, n_fft):
    n = 1 << 22
    x = _noise(n, dtype, n_fft)
    step, K = _welch(n, n_fft, 50)
    check_primitive(x, np.hanning(n_fft), n_fft, step, K, "2^22 %s n_fft %d" % (np.dtype(dtype).name, n_fft))


@pytest.mark.parametrize("dtype", [np.complex64, np.float32])
@pytest.mark.parametrize("kind", ["tone+noise", "tone", "dc"])
def test_coherent_inputs(dtype, kind):
    """Coherent inputs do not average their rounding away: the same bounds hold."""
    n, n_fft = 1 << 22, 1024
    m = np.arange(n)
    if kind == "dc":
        x = np.ones(n, dtype=np.complex128)
    else:
        x = np.exp(2j * np.pi * 200 / n_fft * m)   # bin-centred
        if kind == "tone+noise":
            # 30 dB above the noise in its bin: the Hann-windowed tone's bin holds (n_fft/2)^2 A^2, the noise n_fft 3/8 sigma^2
            sigma = np.sqrt((n_fft / 2) ** 2 / (n_fft * 0.375) / 1000.0)
            x = x + sigma * _noise(n, np.complex128, 30) / np.sqrt(2)
    x = (x if dtype == np.complex64 else x.real).astype(dtype)
    step, K = _welch(n, n_fft, 50)
    check_primitive(x, np.hanning(n_fft), n_fft, step, K, "%s %s" % (kind, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.float64, np.complex128])
def test_non_finite_samples(dtype):
    n_fft, step = 256, 128
    n = 100000
    x = _noise(n, dtype, 9)
    K = 700                                  # the last segment ends at 699 * 128 + 256 = 89728
    w = windows.hann(n_fft)
    assert w[0] == 0.0
    clean = _ffi.psd_accum(x, w, n_fft, step, K)
    assert np.all(np.isfinite(clean))
    xd = _ffi.DeviceArray.from_host(x)
    Sd = _ffi.DeviceArray(n_fft, np.float64)
    _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, K)
    assert np.array_equal(Sd.to_host(), clean)
    # behind the last segment: never read, bit-identical
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[89728] = bad
        xb[-1] = bad
        xd.write(xb)
        _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, K)
        assert np.array_equal(Sd.to_host(), clean)
    # in a used sample: every bin non-finite -- under w[0] = 0 (sample 0 belongs to segment 0 only, at window index 0),
    # in the second segment of a pair, in the very last sample used, in the middle
    for at in (0, 128 + 5, 89727, 44444):
        for bad in (np.nan, np.inf, -np.inf):
            xb = x.copy()
            xb[at] = bad
            S = _ffi.psd_accum(xb, w, n_fft, step, K)
            assert not np.any(np.isfinite(S)), (at, bad)
    if np.dtype(dtype).kind == "c":
        xb = x.copy()
        xb[0] = complex(0.25, np.inf)
        assert not np.any(np.isfinite(_ffi.psd_accum(xb, w, n_fft, step, K)))
    xd.free()
    Sd.free()


@pytest.mark.parametrize("dtype,n_fft", [(np.complex64, 1024), (np.float32, 4096), (np.complex64, 64)])
def test_float32_image_option(dtype, n_fft):
    """Option psd_f32_image (what config.precision = "single" selects): the float32 LDS image, held to the 1e-6 contract only."""
    x = _noise(1 << 22, dtype, 8) + dtype(3) * np.exp(2j * np.pi * 0.125 * np.arange(1 << 22)).real.astype(np.float32)
    step, K = _welch(x.size, n_fft, 50)
    w = windows.hann(n_fft)
    ref = ss.psd_accum_host(x, w, n_fft, step, K)
    S64 = _ffi.psd_accum(x, w, n_fft, step, K)
    with _ffi.option("psd_f32_image", 1):
        S32 = _ffi.psd_accum(x, w, n_fft, step, K)
        assert np.array_equal(S32, _ffi.psd_accum(x, w, n_fft, step, K))
    print("float32 image: peak-relative %.2e, per-bin %.2e; float64 image %.2e, %.2e" % (peak_err(S32, ref), bin_err(S32, ref),
                                                                                    peak_err(S64, ref), bin_err(S64, ref)))
    assert peak_err(S32, ref) <= 1e-6 and not np.array_equal(S32, S64)
    with _cfg(precision="single"):
        real = dtype == np.float32
        P = ss.psd(x.astype(np.float64 if real else np.complex128), n_fft, scale_noise=False)[0]
    Sp = S32[:n_fft // 2 + 1] if real else np.fft.fftshift(S32)
    assert np.array_equal(P, Sp / (K * n_fft ** 2 * (sum(w) / n_fft) ** 2))


def test_two_runs_are_bit_identical():
    for dtype, n_fft in ((np.complex64, 1024), (np.float32, 256), (np.float64, 2048)):
        x = _noise(1 << 22, dtype, 4)
        step, K = _welch(x.size, n_fft, 50)
        w = np.hanning(n_fft)
        a = _ffi.psd_accum(x, w, n_fft, step, K)
        b = _ffi.psd_accum(x, w, n_fft, step, K)
        assert np.array_equal(a, b)
        assert np.array_equal(ss.psd(x, n_fft)[0], ss.psd(x, n_fft)[0])


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.float64, np.complex128])
def test_dev_entry_writes_exactly_n_fft_doubles(dtype):
    guard = 64
    x = _noise(300001, dtype, 5)
    xd = _ffi.DeviceArray.from_host(x)
    for n_fft, ns, step, K in ((64, 64, 32, 9000), (256, 200, 77, 1), (1024, 1024, 512, 500), (4096, 4096, 1024, 200),
                               (128, 128, 1, 3001), (2048, 2048, 2048 * 3, 40)):
        w = np.hanning(ns) + 0.01
        Sd = _ffi.DeviceArray(n_fft + guard, np.float64)
        sentinel = np.full(n_fft + guard, 7.25)
        Sd.write(sentinel)
        _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, K)
        got = Sd.to_host()
        assert np.array_equal(got[n_fft:], sentinel[n_fft:]), (n_fft, ns, step, K)
        ref = ss.psd_accum_host(x, w, n_fft, step, K)
        assert peak_err(got[:n_fft], ref) <= (1e-6 if dtype in (np.float32, np.complex64) else 1e-12), (n_fft, ns, step, K)
        assert np.array_equal(got[:n_fft], _ffi.psd_accum(x, w, n_fft, step, K))
        Sd.free()
    with pytest.raises(ValueError):
        _ffi.psd_accum_dev(xd, _ffi.DeviceArray(100, np.float64), np.ones(256), 256, 128, 4)
    with pytest.raises(ValueError):
        _ffi.psd_accum_dev(xd, _ffi.DeviceArray(256, np.float64), np.ones(256), 256, 128, 1 << 20)
    xd.free()


def test_engine_record_and_host_takeover(caplog):
    x = _noise(50000, np.complex64, 6)
    _ffi.debug_path()
    for n_fft in (64, 128, 256, 512, 1024, 2048, 4096):
        ss.psd(x, n_fft)
        assert _ffi.debug_path() == ["psd"], n_fft
    import logging
    with caplog.at_level(logging.INFO, logger=ss.log.name):
        for n_fft in (1000, 32, 8192):
            Px, _ = ss.psd(x, n_fft)
            assert "psd" not in _ffi.debug_path(), n_fft
            step, K = _welch(x.size, n_fft, 50)
            assert Px.shape == (n_fft,) and K > 0
    assert sum("host" in r.getMessage() for r in caplog.records) >= 3
    f, Sx = ss.simple_sa(x, 128, 512, 1.0, NAVG=5, window="hann")
    assert _ffi.debug_path() == ["psd"] and Sx.shape == (256,)          # complex64: the one-sided branch
    f, Sx = ss.simple_sa(x.astype(np.complex128), 128, 512, 1.0, NAVG=5)
    assert Sx.shape == (512,)
    Px, f = ss.my_psd(x[:700])
    assert _ffi.debug_path() == ["psd"] and Px.shape == (1024,)


@pytest.mark.parametrize("n,ns,n_fft,step,nseg", [(64, 64, 64, 32, 1), (1000, 128, 256, 64, 14), (333, 100, 128, 50, 5)])
def test_host_form_equals_the_device_form_bit_for_bit(n, ns, n_fft, step, nseg):
    """skdsp_psd (host pointers: only the samples the segments reach are staged) against skdsp_psd_dev on the same vector"""
    rng = np.random.default_rng(66 + n)
    w = np.hanning(ns)
    for dtype in (np.float32, np.complex64, np.complex128):
        x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dtype).kind == "c" else 0)).astype(dtype)
        S = _ffi.psd_accum(x, w, n_fft, step, nseg)
        xd, Sd = _ffi.DeviceArray.from_host(x), _ffi.DeviceArray(n_fft, np.float64)
        _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, nseg)
        assert np.any(S > 0) and np.array_equal(Sd.to_host().view(np.uint64), S.view(np.uint64)), dtype
