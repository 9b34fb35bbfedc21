"""Plan ownership of the frequency-domain tile engines (csrc/fir_up4k.hip, fir_up2k.hip, fir_dn4k.hip: per-factor plans a FIR handle
owns, found by key, freed with the handle; csrc/fir_bank.hip: the tables a bank handle owns): several plans on ONE handle, their
lookup, their destruction.

One complex64 and one float32 handle, 96 real low-pass taps, 12 289 samples (three or more tiles of every engine with a ragged last
one; n / M >= 2048 for M = 2, 3).  Every call runs under the option that sends it to the engine it is meant for -- left to the cost
models, a signal this short goes to the polyphase kernels and no plan is ever made -- and the engine is asserted (skdsp_debug_path).

Tolerance: the float32 contract, max |y - ref| <= 1e-6 x peak, as tests/test_gpu_iir_par.py holds the same engines to; ref is the
direct-form convolution in float64 (np.convolve)."""
import contextlib

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, sigsys as ss
from test_caf_cpu import quiet, row_peak_err

pytestmark = pytest.mark.gpu

N = 12289
NTAPS = 96
TOL = 1e-6
_m = np.arange(NTAPS) - (NTAPS - 1) / 2.0
B = 0.2 * np.sinc(0.2 * _m) * np.hamming(NTAPS)   # Hamming-windowed low-pass, unit DC gain
B = B / np.sum(B)

# (what, factor, options, engine): the calls one handle makes, in this order
SEQUENCE = [
    ("up", 3, {"fir_up4k": 2}, "fir_up4k"),                    # first plan of the 4096-point interpolator
    ("up", 10, {"fir_up4k": 2}, "fir_up2k"),                   # five passes or more: first plan of the 2048-point one
    ("up", 10, {"fir_up4k": 2, "fir_up2k": 0}, "fir_up4k"),    # a second plan beside L = 3
    ("up", 3, {"fir_up4k": 2}, "fir_up4k"),                    # found again, behind it
    ("up", 3, {"fir_up4k": 2, "fir_up2k": 2}, "fir_up2k"),     # a second plan beside L = 10
    ("up", 10, {"fir_up4k": 2, "fir_up2k": 2}, "fir_up2k"),    # found again
    ("dn", 2, {"fir_dn4k": 2}, "fir_dn4k"),
    ("dn", 3, {"fir_dn4k": 2}, "fir_dn4k"),
    ("dn", 2, {"fir_dn4k": 2}, "fir_dn4k"),
]


def _signal(dt):
    rng = np.random.default_rng(12289)
    x = rng.standard_normal(N)
    if np.dtype(dt).kind == "c":
        x = (x + 1j * rng.standard_normal(N)) / np.sqrt(2)
    return x.astype(dt)


def _reference(x, what, f):
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if what == "up":
        up = np.zeros(N * f, dtype=xw.dtype)
        up[::f] = f * xw
        return np.convolve(up, B)[:N * f]
    return np.convolve(xw, B)[:N][::f][:N // f]


def _call(k, xd, what, f, opts):
    """(result, engines launched) of one call on handle k"""
    count = N * f if what == "up" else N // f
    yd = _ffi.DeviceArray(count, xd.dtype)
    try:
        _ffi.debug_path()
        with contextlib.ExitStack() as st:
            for name, val in opts.items():
                st.enter_context(_ffi.option(name, val))
            (k.up_dev if what == "up" else k.dn_dev)(xd, yd, f)
        return yd.to_host(), _ffi.debug_path()
    finally:
        yd.free()


@pytest.fixture(scope="module", params=[np.complex64, np.float32], ids=["complex64", "float32"])
def case(request):
    """(dtype, x, {(what, factor): float64 reference}): computed once per dtype"""
    x = _signal(request.param)
    return request.param, x, {(w, f): _reference(x, w, f) for w, f in {(w, f) for w, f, _, _ in SEQUENCE}}


def test_plans_of_one_handle(case):
    dt, x, refs = case
    xd = _ffi.DeviceArray.from_host(x)
    try:
        for cycle in range(2):   # (the second cycle: create / call / destroy works again behind the first handle's destruction)
            k = _ffi.FirKernel(B, _ffi.code_of(dt))
            first = {}
            for step, (what, f, opts, engine) in enumerate(SEQUENCE):
                y, path = _call(k, xd, what, f, opts)
                assert path == [engine], (cycle, step, path)
                ref = refs[(what, f)]
                e = np.max(np.abs(y - ref)) / max(np.max(np.abs(y)), np.max(np.abs(ref)))
                print("%s cycle %d step %d %s by %d through %s: max |y - ref| / peak %.3g" % (np.dtype(dt).name, cycle, step, what, f, engine, e))
                assert e <= TOL, (cycle, step, e)
                # a handle that makes only this call computes the same bytes ...
                fresh = _ffi.FirKernel(B, _ffi.code_of(dt))
                y1, path1 = _call(fresh, xd, what, f, opts)
                fresh._fin()
                assert path1 == [engine] and y.tobytes() == y1.tobytes(), (cycle, step)
                # ... and so did this handle when it first made it
                key = (what, f, engine)
                assert first.setdefault(key, y).tobytes() == y.tobytes(), (cycle, step)
            k._fin()
    finally:
        xd.free()


def test_bank_tables_of_one_handle(case):
    """The bank handle's tables: create / call / destroy twice, 3 bands over the same signal, against sigsys.fft_caf_host (the rows
    of its n_fft2 = 128 blocks: 12 288 of the 12 289 samples)."""
    dt, x, _ = case
    kw = dict(n_fft2=128, n_slice2=1, bs=5.0, fs=256.0)   # slices 5 bins of 256 apart
    ref = quiet(ss.fft_caf_host, x, B, **kw)[0][0][:, :N - 1]
    g = np.conj(B[::-1])
    xd = _ffi.DeviceArray.from_host(x)
    yd = _ffi.DeviceArray(3 * N, np.complex64)
    try:
        outs = []
        for cycle in range(2):
            bank = _ffi.FirBank(g, [-5, 0, 5], 256, dt)
            _ffi.debug_path()
            bank.filter_dev(xd, yd)
            assert _ffi.debug_path() == ["fir_bank4k"]
            y = yd.to_host().reshape(3, N)
            bank._fin()
            e = row_peak_err(y[:, :N - 1].astype(complex), ref)
            print("%s cycle %d bank: worst row max |y - ref| / peak %.3g" % (np.dtype(dt).name, cycle, e))
            assert e <= TOL, (cycle, e)
            outs.append(y)
        assert outs[0].tobytes() == outs[1].tobytes()
    finally:
        xd.free()
        yd.free()
