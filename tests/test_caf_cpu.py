"""sigsys.fft_caf without a GPU: the host float64 restatement (sigsys.fft_caf_host) reproduces the captured reference (g17),
the FIR form the device engines run equals it, the integer phase reduction equals np.roll of the 2 n_fft2-point spectrum
for any shift, the signature, printed lines and errors are the reference's, and the public fft_caf settles every argument
convention before any device call."""
import contextlib
import inspect
import io
import json
import os

import numpy as np
import pytest
import scipy.signal as signal

from sk_dsp_comm_amd import _ffi, sigsys as ss
from conftest import GOLDEN


def g17_cases():
    g = np.load(os.path.join(GOLDEN, "g17_caf.npz"))
    return g, json.loads(str(g["cases"]))


def quiet(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        r = fn(*a, **kw)
    return r, buf.getvalue()


def row_peak_err(y, ref):
    """worst over the rows of max |y - ref| / max |ref| (rows that are all zero must be reproduced exactly)"""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    worst = 0.0
    for a, b in zip(y, ref):
        peak = float(np.max(np.abs(b))) if b.size else 0.0
        d = float(np.max(np.abs(a - b))) if b.size else 0.0
        worst = max(worst, d / peak if peak > 0 else (0.0 if d == 0 else np.inf))
    return worst


def conventions():
    return json.load(open(os.path.join(GOLDEN, "g17_conventions.json")))


def test_host_restatement_reproduces_reference_g17():
    g, cases = g17_cases()
    assert {c["key"] for c in cases} >= {"real300", "cplx65", "full2049", "wrap100", "slice0", "onetap", "cplxref", "ragged"}
    worst = 0.0
    for c in cases:
        k = c["key"]
        (y, f, t), out = quiet(ss.fft_caf_host, g[k + "_x"], g[k + "_h"], **c["args"])
        assert y.dtype == np.complex128 and f.dtype == t.dtype == np.float64, k
        e = row_peak_err(y, g[k + "_y"])
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
        assert f.shape == g[k + "_f"].shape and np.allclose(f, g[k + "_f"], rtol=1e-15, atol=0), k
        assert t.shape == g[k + "_t"].shape and np.allclose(t, g[k + "_t"], rtol=1e-15, atol=0), k
        assert out == str(g[k + "_out"]), k
        F = c["args"]["n_fft2"]
        n_use = (len(g[k + "_x"]) // F) * F
        assert not np.any(y[:, n_use:]), k          # the tail behind the last whole block stays zero
    print("worst row-peak-relative error of fft_caf_host against the reference: %.2e" % worst)


def test_fir_form_equals_the_block_fft_form():
    """y[j, m] = sum_n g_j[n] x[m - n] with g_j = _caf_band_taps(conj(h[::-1]), s_j, 2 F): what the device engines compute."""
    g, cases = g17_cases()
    worst = 0.0
    for c in cases:
        k = c["key"]
        x, h, a = g[k + "_x"], g[k + "_h"], c["args"]
        F, ns2 = a["n_fft2"], a.get("n_slice2", 0)
        step = round(a.get("bs", 0.1) * 2 * F / a.get("fs", 1.0))
        n_use = (len(x) // F) * F
        ref = g[k + "_y"]
        y = np.zeros_like(ref)
        for j in range(2 * ns2 + 1):
            y[j, :n_use] = signal.lfilter(ss._caf_band_taps(np.conj(h[::-1]), (j - ns2) * step, 2 * F), 1.0, x[:n_use].astype(complex))
        e = row_peak_err(y, ref)
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print("worst row-peak-relative error of the FIR form against the reference: %.2e" % worst)


def test_integer_phase_reduction_matches_roll_of_the_spectrum():
    rng = np.random.default_rng(17)
    for F, P in ((100, 40), (128, 128), (1000, 300), (7, 7)):
        gt = rng.standard_normal(P) + 1j * rng.standard_normal(P)
        H = np.fft.fft(gt, 2 * F)
        scale = float(np.max(np.abs(H)))
        for s in (0, 1, -1, F, 2 * F - 1, 2 * F, -2 * F, 2 * F + 3, -5 * F - 1, 240, -240, 10 ** 12 + 7, -(10 ** 12) - 7):
            Hs = np.fft.fft(ss._caf_band_taps(gt, s, 2 * F), 2 * F)
            assert np.max(np.abs(Hs - np.roll(H, s))) <= 1e-13 * scale, (F, P, s)
        # the reduced phase is EXACTLY periodic in the shift: beyond +-2F nothing changes, to the bit
        assert np.array_equal(ss._caf_band_taps(gt, 2 * F + 3, 2 * F), ss._caf_band_taps(gt, 3, 2 * F))
        assert np.array_equal(ss._caf_band_taps(gt, -4 * F - 3, 2 * F), ss._caf_band_taps(gt, 2 * F - 3, 2 * F))


def test_signature_prints_and_errors_match_reference():
    conv = conventions()
    sig = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in inspect.signature(ss.fft_caf).parameters.values()]
    assert sig == conv["signature"]
    assert [p for p in inspect.signature(ss.fft_caf_host).parameters] == [s[0] for s in sig]
    xr = np.random.default_rng(2).standard_normal(600)
    h = np.ones(20)
    for fn in (ss.fft_caf, ss.fft_caf_host):
        with pytest.raises(ValueError) as ei:
            fn(xr, h, n_fft2=19)
        assert conv["h_too_long"] == {"raises": "ValueError", "message": str(ei.value)}
        (y, f, t), out = quiet(fn, xr[:50], h, n_fft2=64, n_slice2=1)      # shorter than one block: all zeros, no device work
        want = conv["x_short"]
        assert out == want["stdout"] and list(y.shape) == want["y"]["shape"] and str(y.dtype) == want["y"]["dtype"] and not np.any(y)
        assert list(f.shape) == want["f"]["shape"] and list(t.shape) == want["t"]["shape"]


def test_conventions_are_settled_before_any_device_call(monkeypatch):
    """The device work of fft_caf is one function; with it replaced by one that raises, everything that raises the reference's
    error, or returns without needing a block, never got that far -- and what does need the device reaches it with the arguments
    the conventions promise."""
    conv = conventions()
    seen = []

    def device(x_use, g, shifts, period, y):
        seen.append((x_use.dtype, x_use.shape, len(g), list(shifts), period, y.shape))
        raise RuntimeError("device route")

    monkeypatch.setattr(ss, "_caf_rows", device)
    xr = np.random.default_rng(3).standard_normal(600)
    h = np.random.default_rng(4).standard_normal(20)
    for name, arg in (("x_list", list(xr)), ("x_tuple", tuple(xr))):
        with pytest.raises(TypeError) as ei, contextlib.redirect_stdout(io.StringIO()):
            ss.fft_caf(arg, h, n_fft2=64)
        assert conv[name] == {"raises": "TypeError", "message": str(ei.value)}, name
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        ss.fft_caf(xr.reshape(2, 300), h, n_fft2=64)                     # deliberate: one-dimensional input only
    assert conv["x_2d"]["y"]["shape"] == [1, 2] and "x_2d" in conv["deliberate_differences"]
    with pytest.raises(ValueError):
        ss.fft_caf(xr, h, n_fft2=19)
    for name, arg, kw in (("x_list_short", list(xr[:50]), {}), ("x_short", xr[:50], {"n_slice2": 1}), ("x_empty", np.zeros(0), {})):
        (y, f, t), out = quiet(ss.fft_caf, arg, h, n_fft2=64, **kw)
        want = conv[name]
        assert out == want["stdout"], name
        assert list(y.shape) == want["y"]["shape"] and str(y.dtype) == want["y"]["dtype"] and not np.any(y), name
        assert list(f.shape) == want["f"]["shape"] and list(t.shape) == want["t"]["shape"], name
    assert seen == []
    # what does reach the device: integers as float64, lists of reference samples as arrays, whole blocks only, period 2 n_fft2
    for name, xa, ha in (("x_int64", np.arange(600) % 17, h), ("h_list", xr, list(h)), ("h_int64", xr, np.arange(20) % 5),
                         ("x_float32", xr.astype(np.float32), h)):
        assert "raises" not in conv[name] and conv[name]["y"]["shape"] == [1, 600], name
        with pytest.raises(RuntimeError, match="device route"), contextlib.redirect_stdout(io.StringIO()):
            ss.fft_caf(xa, ha, n_fft2=64)
        dt, shape, P, shifts, period, yshape = seen.pop()
        assert dt == (np.float32 if name == "x_float32" else np.float64) and shape == (576,), name
        assert (P, shifts, period, yshape) == (20, [0], 128, (1, 600)), name
    with pytest.raises(RuntimeError, match="device route"), contextlib.redirect_stdout(io.StringIO()):
        ss.fft_caf(xr + 0j, h, n_fft2=100, n_slice2=4, bs=0.3, fs=1.0)
    assert seen.pop()[3] == [-240, -180, -120, -60, 0, 60, 120, 180, 240]


def test_bank_abi_rejects_bad_arguments_without_a_device():
    ok = dict(taps=np.ones(8), shifts=[0, 1], period=16, dtype=np.complex64)
    for bad in (dict(taps=np.ones(2050)),              # ntaps - 1 > 2048
                dict(shifts=[]),                       # nbands < 1
                dict(period=0),                        # period < 1
                dict(taps=np.ones(2049), shifts=np.zeros(5000, np.int64)),   # tables above the byte cap
                dict(dtype=np.float64), dict(dtype=np.complex128)):
        with pytest.raises(ValueError):
            _ffi.FirBank(**{**ok, **bad})
    with pytest.raises(ValueError):
        _ffi.FirBank(np.ones((2, 4)), [0], 16, np.complex64)
