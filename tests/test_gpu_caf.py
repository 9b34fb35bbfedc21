"""sigsys.fft_caf on the MI355X: the captured reference (g17) on the default float64 route and, cast to float32 / complex64,
through the fused bank kernel (csrc/fir_bank.hip); tile edges, band grouping, the tap limits, the precision switches,
non-finite samples, determinism and the raw _ffi.FirBank entry point.

Tolerances: float64 / complex128 signals 1e-12, float32 / complex64 signals 1e-6 (the project's float32 contract), both as
max |y - ref| over a row against that row's peak |ref|.  Where no fixture reaches, ref is sigsys.fft_caf_host."""
import ctypes
import logging

import numpy as np
import pytest
import scipy.signal as signal

from sk_dsp_comm_amd import _ffi, config, sigsys as ss
from test_caf_cpu import g17_cases, quiet, row_peak_err

pytestmark = pytest.mark.gpu

BANK = "fir_bank4k"


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


def single(x):
    return x.astype(np.complex64 if np.iscomplexobj(x) else np.float32)


def noise(rng, n, cplx):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


def caf(x, h, **kw):
    """(y, engines the call launched) of the public function, its prints swallowed"""
    _ffi.debug_path()
    (y, f, t), _ = quiet(ss.fft_caf, x, h, **kw)
    return y, _ffi.debug_path()


def host(x, h, **kw):
    return quiet(ss.fft_caf_host, x, h, **kw)[0][0]


def test_g17_float64_default_route():
    g, cases = g17_cases()
    worst = 0.0
    for c in cases:
        k = c["key"]
        _ffi.debug_path()
        (y, f, t), out = quiet(ss.fft_caf, g[k + "_x"], g[k + "_h"], **c["args"])
        assert BANK not in _ffi.debug_path(), k
        assert y.dtype == np.complex128 and out == str(g[k + "_out"]), k
        assert np.allclose(f, g[k + "_f"], rtol=1e-15, atol=0) and np.allclose(t, g[k + "_t"], rtol=1e-15, atol=0), k
        e = row_peak_err(y, g[k + "_y"])
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print("g17, float64 route: worst row error %.2e" % worst)


def test_g17_single_precision_through_the_bank():
    """Every g17 case cast to float32 / complex64 (len(h_ref) = 2049 = n_fft2 and len(h_ref) = 1 among them)."""
    g, cases = g17_cases()
    worst = worst_walk = 0.0
    with _cfg(strict_dtype=False):
        for c in cases:
            k = c["key"]
            x, h, a = single(g[k + "_x"]), g[k + "_h"], c["args"]
            y, path = caf(x, h, **a)
            assert BANK in path, (k, path)
            assert y.dtype == np.complex128 and y.shape == g[k + "_y"].shape, k
            e = row_peak_err(y, g[k + "_y"])
            # the per-band route on the same input, for comparison
            F, ns2 = a["n_fft2"], a.get("n_slice2", 0)
            step = round(a.get("bs", 0.1) * 2 * F / a.get("fs", 1.0))
            n_use = (len(x) // F) * F
            yw = np.zeros_like(y)
            gt = np.conj(h[::-1])
            ss._band_walk(x[:n_use], np.complex64, lambda j: ss._caf_band_taps(gt, (j - ns2) * step, 2 * F), 2 * ns2 + 1, yw)
            ew = row_peak_err(yw, g[k + "_y"])
            print("g17 %-9s bank %.2e   per-band walk %.2e" % (k, e, ew))
            worst, worst_walk = max(worst, e), max(worst_walk, ew)
            assert e <= 1e-6, (k, e)
    print("g17, float32 / complex64: worst row error bank %.2e, per-band walk %.2e" % (worst, worst_walk))


@pytest.fixture(scope="module")
def edge_signals():
    """F = 1000, P = 300 (overlap 512, 3584 outputs per tile), 12345 samples: three whole tiles, a partial one, a zero tail of 345."""
    rng = np.random.default_rng(1701)
    return {"h": noise(rng, 300, False), "r": single(noise(rng, 12345, False)), "c": single(noise(rng, 12345, True))}


@pytest.mark.parametrize("kind", ["r", "c"])
def test_tile_edges(edge_signals, kind):
    x, h = edge_signals[kind], edge_signals["h"]
    kw = dict(n_fft2=1000, n_slice2=3, bs=0.5, fs=1000.0)
    with _cfg(strict_dtype=False):
        y, path = caf(x, h, **kw)
    assert BANK in path
    assert y.shape == (7, 12345) and not np.any(y[:, 12000:])
    e = row_peak_err(y, host(x, h, **kw))
    print("tile edges (%s): %.2e" % (x.dtype, e))
    assert e <= 1e-6


def test_band_groups_short_signal_many_slices(edge_signals):
    """81 rows over four tiles: the bands are split into groups so that the grid fills the device."""
    x, h = edge_signals["c"], edge_signals["h"]
    kw = dict(n_fft2=1000, n_slice2=40, bs=0.5, fs=1000.0)
    with _cfg(strict_dtype=False):
        y, path = caf(x, h, **kw)
    assert BANK in path and y.shape == (81, 12345)
    e = row_peak_err(y, host(x, h, **kw))
    print("81 slices, 12345 samples: %.2e" % e)
    assert e <= 1e-6


def test_band_groups_long_signal_few_slices(edge_signals):
    """2^20 samples, 9 slices: the tiles alone fill the grid, so one group holds all bands."""
    rng = np.random.default_rng(1702)
    x = single(noise(rng, 1 << 20, True))
    kw = dict(n_fft2=1000, n_slice2=4, bs=0.5, fs=1000.0)
    with _cfg(strict_dtype=False):
        y, path = caf(x, edge_signals["h"], **kw)
    assert BANK in path and y.shape == (9, 1 << 20)
    e = row_peak_err(y, host(x, edge_signals["h"], **kw))
    print("9 slices, 2^20 samples: %.2e" % e)
    assert e <= 1e-6


def test_every_grouping_gives_the_same_rows(edge_signals):
    """Option fir_bank_per forces the bands per group: one band per item, ragged groups and one group give identical bytes
    (a band's arithmetic does not depend on which workgroup runs it)."""
    x, h = edge_signals["c"], edge_signals["h"]
    kw = dict(n_fft2=1000, n_slice2=5, bs=0.5, fs=1000.0)
    with _cfg(strict_dtype=False):
        ref, path = caf(x, h, **kw)
        assert BANK in path
        for per in (1, 4, 11, 100):
            with _ffi.option("fir_bank_per", per):
                y, _ = caf(x, h, **kw)
            assert y.tobytes() == ref.tobytes(), per


def test_tap_limits(caplog):
    rng = np.random.default_rng(1703)
    with _cfg(strict_dtype=False):
        for P, F, n in ((2049, 2049, 3 * 2049 + 5), (1, 64, 1000)):        # served: overlap 2048 and overlap 0
            x, h = single(noise(rng, n, True)), noise(rng, P, True)
            kw = dict(n_fft2=F, n_slice2=1, bs=0.3, fs=1.0)
            y, path = caf(x, h, **kw)
            assert BANK in path, (P, path)
            e = row_peak_err(y, host(x, h, **kw))
            print("P = %d: %.2e" % (P, e))
            assert e <= 1e-6, (P, e)
        x, h = single(noise(rng, 7000, True)), noise(rng, 3000, False)     # longer than the tile serves: one FIR pass per slice
        kw = dict(n_fft2=3000, n_slice2=1, bs=0.3, fs=1.0)
        with caplog.at_level(logging.INFO, logger=ss.log.name):
            y, path = caf(x, h, **kw)
        assert BANK not in path and path, path
        assert any("one FIR pass per slice" in r.getMessage() for r in caplog.records)
        e = row_peak_err(y, host(x, h, **kw))
        print("P = 3000 (per-band route): %.2e" % e)
        assert e <= 1e-6, e


def test_precision_switches(edge_signals):
    h = edge_signals["h"]
    kw = dict(n_fft2=1000, n_slice2=1, bs=0.5, fs=1000.0)
    x64 = edge_signals["c"][:5000].astype(np.complex128)
    ref = host(x64, h, **kw)
    with _cfg(precision="single"):                     # float64 input, precision "single": the bank kernel
        y, path = caf(x64, h, **kw)
    assert BANK in path and row_peak_err(y, ref) <= 1e-6
    with _cfg(strict_dtype=True):                      # float32 input under strict_dtype: not the bank kernel
        y, path = caf(edge_signals["r"][:5000], h, **kw)
    assert BANK not in path and path
    assert row_peak_err(y, host(edge_signals["r"][:5000], h, **kw)) <= 1e-12
    with _cfg(strict_dtype=False, precision="double"):
        y, path = caf(edge_signals["c"][:5000], h, **kw)
    assert BANK not in path and row_peak_err(y, ref) <= 1e-12
    y, path = caf(x64, h, **kw)                        # float64 input by default
    assert BANK not in path and row_peak_err(y, ref) <= 1e-12


@pytest.mark.parametrize("kind", ["c", "r"])
def test_non_finite_samples_stay_local(edge_signals, kind):
    """inf at 5000 (the middle of tile 1) and nan at 7100 (68 samples in front of the edge between tiles 1 and 2: it poisons both):
    in every row only the P = 300 outputs that multiply each sample are non-finite."""
    x, h = edge_signals[kind][:12000].copy(), edge_signals["h"]
    P = len(h)
    kw = dict(n_fft2=1000, n_slice2=3, bs=0.5, fs=1000.0)
    x[5000], x[7100] = np.inf, np.nan
    clean = x.copy()
    clean[[5000, 7100]] = 0
    ref = host(clean, h, **kw)
    with _cfg(strict_dtype=False):
        y, path = caf(x, h, **kw)
    assert BANK in path
    hit = np.zeros(12000, bool)
    hit[5000:5000 + P] = hit[7100:7100 + P] = True
    assert np.all(~np.isfinite(y[:, hit])), "outputs that multiply a non-finite sample must be non-finite"
    assert np.all(np.isfinite(y[:, ~hit]))
    e = row_peak_err(y[:, ~hit], ref[:, ~hit])
    print("non-finite (%s): finite part %.2e" % (x.dtype, e))
    assert e <= 1e-6


def test_row_offsets_beyond_2_to_31_elements(edge_signals):
    """Rows 2^30 + 8 elements apart: row 2 starts past element 2^31 of y (the 17 GB between the rows are never touched)."""
    x = edge_signals["c"][:5000]
    g = np.conj(edge_signals["h"][::-1])
    shifts, n, stride = [-3, 0, 5], 5000, (1 << 30) + 8
    xd = _ffi.DeviceArray.from_host(x)
    yd = _ffi.DeviceArray(2 * stride + n, np.complex64)
    try:
        _ffi.FirBank(g, shifts, 2000, np.complex64).filter_dev(xd, yd, stride)
        y = np.stack([yd.to_host(j * stride, n) for j in range(3)])
    finally:
        xd.free()
        yd.free()
    ref = np.stack([signal.lfilter(ss._caf_band_taps(g, s, 2000), 1.0, x.astype(complex)) for s in shifts])
    assert row_peak_err(y.astype(complex), ref) <= 1e-6


def test_two_calls_give_identical_bytes(edge_signals):
    kw = dict(n_fft2=1000, n_slice2=40, bs=0.5, fs=1000.0)
    with _cfg(strict_dtype=False):
        y1, _ = caf(edge_signals["c"], edge_signals["h"], **kw)
        y2, _ = caf(edge_signals["c"], edge_signals["h"], **kw)
    assert y1.tobytes() == y2.tobytes()


def test_raw_bank_row_stride_and_bad_arguments(edge_signals):
    x = edge_signals["c"][:9000]
    g = np.conj(edge_signals["h"][::-1])
    shifts, n, stride = [-3, 0, 5], 9000, 9100
    bank = _ffi.FirBank(g, shifts, 2000, np.complex64)
    xd = _ffi.DeviceArray.from_host(x)
    sentinel = np.complex64(-7.5 + 2.25j)
    yd = _ffi.DeviceArray.from_host(np.full(3 * stride, sentinel, np.complex64))
    try:
        _ffi.debug_path()
        bank.filter_dev(xd, yd, stride)
        assert _ffi.debug_path() == [BANK]
        y = yd.to_host().reshape(3, stride)
        assert np.all(y[:, n:] == sentinel), "the gap between two rows must stay untouched"
        ref = np.stack([signal.lfilter(ss._caf_band_taps(g, s, 2000), 1.0, x.astype(complex)) for s in shifts])
        assert row_peak_err(y[:, :n].astype(complex), ref) <= 1e-6
        with pytest.raises(ValueError):
            bank.filter_dev(xd, yd, n - 1)
        with pytest.raises(ValueError):
            bank.filter_dev(xd, yd, 2 * stride)
        with pytest.raises(ValueError):
            bank.filter_dev(xd, yd, stride, n=n + 1)
        with pytest.raises(ValueError):
            _ffi.FirBank(g, shifts, 2000, np.float32).filter_dev(xd, yd, stride)            # a complex64 signal through a float32 bank
        lib = _ffi.load()
        with pytest.raises(ValueError):                                                     # the C entry point itself: row_stride < n
            _ffi.check(lib.skdsp_fir_bank_dev(ctypes.c_void_p(bank.h), ctypes.c_void_p(xd.ptr), n, ctypes.c_void_p(yd.ptr), n - 1))
        with pytest.raises(ValueError):                                                     # not a bank handle
            fir = _ffi.FirKernel(g, _ffi.code_of(np.complex64))
            _ffi.check(lib.skdsp_fir_bank_dev(ctypes.c_void_p(fir.h), ctypes.c_void_p(xd.ptr), n, ctypes.c_void_p(yd.ptr), stride))
    finally:
        xd.free()
        yd.free()
    for bad in (dict(taps=np.ones(2050)), dict(shifts=[]), dict(period=0)):
        with pytest.raises(ValueError):
            _ffi.FirBank(**{**dict(taps=g, shifts=shifts, period=2000, dtype=np.complex64), **bad})
