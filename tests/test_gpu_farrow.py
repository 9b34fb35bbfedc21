"""digitalcom.farrow_resample on the MI355X (csrc/farrow.hip): the captured reference (g15), the full-size workloads against
the vectorised restatement (test_farrow_cpu.farrow_restated), windows of the device entry point, non-finite samples, dtypes
and launch-to-launch determinism."""
import json
import os

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, config, digitalcom as dc
from conftest import GOLDEN, rel_err
from test_farrow_cpu import farrow_restated

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


def _peak_err(y, ref):
    return float(np.max(np.abs(y.astype(np.complex128) - ref))) / max(float(np.max(np.abs(ref))), 1e-300) if ref.size else 0.0


def test_g15_through_gpu():
    g = np.load(os.path.join(GOLDEN, "g15_farrow.npz"))
    cases = json.loads(str(g["cases"]))
    _ffi.debug_path()
    for c in cases:
        x, ref = g[c["x"]], g[c["key"]]
        args = (c["fs_old"], c["fs_new"], c["i_ord"], c["alpha"])
        y = dc.farrow_resample(x, *args)
        assert y.shape == ref.shape and y.dtype == ref.dtype, c
        narrow = x.dtype in (np.float32, np.complex64)
        if not narrow and c["i_ord"] == 1:
            assert np.array_equal(y, ref), c
        elif not narrow:
            assert _peak_err(y, ref) <= 1e-12, c
        else:
            assert rel_err(y, ref)[0] <= 1e-6, c
            with _cfg(precision="double"):
                yd = dc.farrow_resample(x, *args)
            assert yd.dtype == ref.dtype
            if c["i_ord"] == 1:
                assert np.array_equal(yd, ref), c
            else:
                assert _peak_err(yd, ref) <= 1e-12, c
    assert "farrow" in _ffi.debug_path()


def test_conventions_with_outputs():
    conv = json.load(open(os.path.join(GOLDEN, "g15_conventions.json")))
    x10 = np.arange(10.0)
    for name, x, fs in (("len3", np.ones(3), (8, 18)), ("both_negative", x10, (-8, -18)), ("float32", x10.astype(np.float32), (8, 18)),
                        ("complex64", x10.astype(np.complex64), (8, 18))):
        y = dc.farrow_resample(x, *fs)
        assert len(y) == conv[name]["len"] and str(y.dtype) == conv[name]["dtype"], name
    assert np.array_equal(dc.farrow_resample(x10, -8, -18), dc.farrow_resample(x10, 8, 18))
    # deliberate difference: integer arrays run as float64
    assert np.array_equal(dc.farrow_resample(np.arange(10), 8, 18, i_ord=1), dc.farrow_resample(x10, 8, 18, i_ord=1))


def _rng_signal(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dtype)


def _chunked_check(x, fs_old, fs_new, i_ord, y, tol, exact=False):
    step = 1 << 24
    for n0 in range(0, y.size, step):
        cnt = min(step, y.size - n0)
        ref = farrow_restated(x, fs_old, fs_new, i_ord, 0.5, n0, cnt)
        if exact:
            assert np.array_equal(y[n0:n0 + cnt], ref), n0
        else:
            d = float(np.max(np.abs(y[n0:n0 + cnt] - ref)))
            assert d <= tol * float(np.max(np.abs(x))), (n0, d)


@pytest.mark.parametrize("dtype,fs_old,fs_new,i_ord,tol", [
    (np.complex64, 48000, 44100, 3, 1e-6),    # W1
    (np.float32, 8, 18, 3, 1e-6),             # W2
    (np.float64, 1, np.pi, 3, 1e-12),         # W3
    (np.float64, 8, 18, 1, 0.0),              # i_ord=1 float64: bit-identical at scale (n_old and mu exact)
])
def test_full_size_workloads(dtype, fs_old, fs_new, i_ord, tol):
    n = 1 << 26
    x = _rng_signal(n, dtype, 26)
    y = dc.farrow_resample(x, fs_old, fs_new, i_ord=i_ord)
    assert y.size == dc._farrow_len(n, 1 / fs_old, 1 / fs_new)
    assert y.dtype == np.result_type(dtype, np.float64)
    _chunked_check(x, fs_old, fs_new, i_ord, y, tol, exact=tol == 0.0)


@pytest.mark.parametrize("dtype,fs_old,fs_new", [(np.float64, 48000, 44100), (np.complex64, 8, 18), (np.complex128, 1, np.pi),
                                                  (np.float32, 20, 1)])   # (20 -> 1: the span outgrows LDS, taps from global memory)
def test_dev_windows_equal_slices_of_the_whole(dtype, fs_old, fs_new):
    n = 400009
    x = _rng_signal(n, dtype, 5)
    xd = _ffi.DeviceArray.from_host(x)
    N = _ffi.farrow_len(n, 1 / fs_old, 1 / fs_new)
    full_d = _ffi.DeviceArray(N, dtype)
    _ffi.farrow_dev(xd, full_d, 1 / fs_old, 1 / fs_new, 3, 0.5)
    full = full_d.to_host()
    assert rel_err(full, farrow_restated(x, fs_old, fs_new, 3))[0] <= (1e-6 if dtype in (np.float32, np.complex64) else 1e-12)
    guard = 64
    for n0, count in ((0, 1), (0, 2049), (1, 2047), (2047, 2), (4095, 4098), (5000, 777), (N - 3, 3), (N - 1, 1), (N // 2, N // 2 - 1), (12345, 0)):
        yd = _ffi.DeviceArray(count + guard, dtype)
        sentinel = np.full(count + guard, 7.25, dtype=dtype)
        yd.write(sentinel)
        _ffi.farrow_dev(xd, yd, 1 / fs_old, 1 / fs_new, 3, 0.5, n0=n0, count=count)
        got = yd.to_host()
        assert np.array_equal(got[:count], full[n0:n0 + count]), (n0, count)
        assert np.array_equal(got[count:], sentinel[count:]), (n0, count)
        yd.free()
    with pytest.raises(ValueError):
        _ffi.farrow_dev(xd, _ffi.DeviceArray(8, dtype), 1 / fs_old, 1 / fs_new, 3, 0.5, n0=N - 4, count=8)


@pytest.mark.parametrize("i_ord", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_non_finite_samples_propagate_exactly(i_ord, dtype):
    n = 5000
    x = _rng_signal(n, dtype, 11)
    clean = dc.farrow_resample(x, 48000, 44100, i_ord=i_ord)
    xb = x.copy()
    xb[1000] = np.inf
    xb[3001] = np.nan
    if np.dtype(dtype).kind == "c":
        xb[2000] = complex(0.5, np.inf)
    y = dc.farrow_resample(xb, 48000, 44100, i_ord=i_ord)
    ref = farrow_restated(xb, 48000, 44100, i_ord)
    bad = ~np.isfinite(ref)
    assert bad.sum() >= 6
    assert np.array_equal(~np.isfinite(y), bad)
    assert np.array_equal(y[~bad], clean[~bad])


def test_narrow_dtypes_and_determinism():
    x = _rng_signal(300001, np.complex64, 3)
    with _cfg(strict_dtype=False):
        y1 = dc.farrow_resample(x, 48000, 44100)
        y2 = dc.farrow_resample(x, 48000, 44100)
        assert y1.dtype == np.complex64
        assert dc.farrow_resample(x.real.copy(), 8, 18).dtype == np.float32
        assert dc.farrow_resample(x.real.astype(np.float64), 8, 18).dtype == np.float64
    assert np.array_equal(y1, y2)
    assert rel_err(y1, farrow_restated(x, 48000, 44100))[0] <= 1e-6
    w1 = dc.farrow_resample(x, 48000, 44100)
    assert w1.dtype == np.complex128 and np.array_equal(w1, dc.farrow_resample(x, 48000, 44100))


@pytest.mark.parametrize("n", [4, 37, 400])
def test_host_form_equals_the_device_form_bit_for_bit(n):
    """skdsp_farrow (host pointers) against skdsp_farrow_dev over the whole output, every order, narrow and wide results"""
    rng = np.random.default_rng(67 + n)
    for dtype in (np.float32, np.complex64, np.float64):
        x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dtype).kind == "c" else 0)).astype(dtype)
        xd = _ffi.DeviceArray.from_host(x)
        for i_ord in (1, 2, 3):
            for wide in (False, True):
                y = _ffi.farrow(x, 1 / 8000.0, 1 / 11025.0, i_ord, wide=wide)
                yd = _ffi.DeviceArray(max(y.size, 1), y.dtype)
                _ffi.farrow_dev(xd, yd, 1 / 8000.0, 1 / 11025.0, i_ord, wide=wide)
                assert y.size == _ffi.farrow_len(n, 1 / 8000.0, 1 / 11025.0) > 0 and yd.to_host(0, y.size).tobytes() == y.tobytes(), (dtype, i_ord, wide)
