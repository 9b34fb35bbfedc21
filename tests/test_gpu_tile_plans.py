"""Plan ownership (csrc/dev_mem.hpp: every table a handle owns is a DevTable or a DevBuffer, every per-shape plan lives in a keyed cache
of its handle and is freed with it): several plans of every cache on ONE handle, their lookup, their destruction.  The FIR caches: the
frequency-domain tile engines (fir_up4k.hip, fir_up2k.hip, fir_dn4k.hip), the polyphase banks and sliding-window tables (fir_direct.hip),
the matrix-pipe tables (fir_mm.hip, fir_bx.hip), the overlap-save plans of .filter and of the walks (fir_ols.hip: kinds 0, 1 + 2, 3) and
their float64 twins (fir_ols64.hip); csrc/fir_bank.hip: the tables a bank handle owns; the IIR plans, tables and grow-only buffers
(test_iir_plans_of_one_handle).

One complex64 and one float32 handle, 96 real low-pass taps, 12 289 samples (three or more tiles of every engine with a ragged last
one; n / M >= 2048 for M = 2, 3).  Every call runs under the option that sends it to the engine it is meant for -- left to the cost
models, a signal this short goes to the polyphase kernels and no plan is ever made -- and the engine is asserted (skdsp_debug_path).

Tolerance: the float32 contract, max |y - ref| <= 1e-6 x peak, as tests/test_gpu_iir_par.py holds the same engines to (float64 and
complex128 handles: the float64 contract of tests/test_gpu_parity.py, 1e-11 x peak); ref is the direct-form convolution in float64
(np.convolve), for the IIR handles scipy.signal.sosfilt in float64."""
import contextlib

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, sigsys as ss
from test_caf_cpu import quiet, row_peak_err

pytestmark = pytest.mark.gpu

N = 12289
NTAPS = 96
TOL = 1e-6
TOL64 = 1e-11
_m = np.arange(NTAPS) - (NTAPS - 1) / 2.0
B = 0.2 * np.sinc(0.2 * _m) * np.hamming(NTAPS)   # Hamming-windowed low-pass, unit DC gain
B = B / np.sum(B)

_POLY = {"fir_up_ols_min": 0, "fir_up4k": 0}                                         # .up never through a frequency-domain engine
_WALK = {"fir_up_ols_min": -1, "fir_up4k": 0, "fir_up_rep": 0, "fir_up_rows_min": 0}   # .up through the walk over (tile, phase) pairs, strided stores
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
    # the older caches, interleaved.  _POLY: never the frequency domain; without the matrix pipe the polyphase launcher's own kernels run
    ("up", 3, {"fir_mm": 0, **_POLY}, "fir_direct"),           # bank L = 3, sliding-window table (3, 1, R)
    ("up", 3, _POLY, "fir_bx"),                                # fp16-piece matrix-pipe table (3, 1)
    ("up", 3, {"fir_bx": 0, **_POLY}, "fir_mm"),               # FP32 matrix-pipe table (3, 1)
    ("up", 5, {"fir_mm": 0, **_POLY}, "fir_direct"),           # a second bank and a second sliding-window table
    ("dn", 2, _POLY, "fir_bx"),                                # a second table (1, 2)
    ("dn", 2, {"fir_bx": 0, **_POLY}, "fir_mm"),               # a second table (1, 2)
    ("updn", (3, 2), {"fir_mm": 0, **_POLY}, "fir_direct"),    # bank L = 3 again, a third sliding-window table (3, 2, R)
    ("filter", 1, {"fir_algo": 2}, "fir_ols"),                 # the overlap-save plan: kind 0, L = 1
    ("up", 3, _WALK, "fir_ols_up"),                            # walk plans beside it: kind 0, L = 3
    ("up", 7, _WALK, "fir_ols_up"),                            # kind 0, L = 7 (float32: phases in pairs, kinds 1 + 2)
    ("up", 4, {"fir_up_rep": 2}, "fir_ols_rep"),               # kind 3, L = 4
    ("up", 3, {"fir_mm": 0, **_POLY}, "fir_direct"),           # all found again, behind what was made since
    ("up", 3, _POLY, "fir_bx"),
    ("up", 3, {"fir_bx": 0, **_POLY}, "fir_mm"),
    ("dn", 2, _POLY, "fir_bx"),
    ("updn", (3, 2), {"fir_mm": 0, **_POLY}, "fir_direct"),
    ("up", 3, _WALK, "fir_ols_up"),
    ("filter", 1, {"fir_algo": 2}, "fir_ols"),
    ("up", 7, _WALK, "fir_ols_up"),
    ("up", 4, {"fir_up_rep": 2}, "fir_ols_rep"),
]
# the float64 overlap-save plans on a complex128 / float64 handle: the filter itself, walks unpaired and (float64, even L) paired
SEQUENCE64 = [
    ("filter", 1, {"fir_algo": 2}, "fir_ols64"),
    ("up", 4, {"fir_up_ols_min": -1}, "fir_ols64_up"),                      # float64: phases in pairs, key (1, 4)
    ("up", 3, {"fir_up_ols_min": -1}, "fir_ols64_up"),                      # unpaired, key (0, 3)
    ("up", 4, {"fir_up_ols_min": -1, "fir_up_pair": 0}, "fir_ols64_up"),    # unpaired beside the pairs of the same L: key (0, 4)
    ("up", 4, {"fir_up_ols_min": -1}, "fir_ols64_up"),                      # each found again
    ("filter", 1, {"fir_algo": 2}, "fir_ols64"),
    ("up", 3, {"fir_up_ols_min": -1}, "fir_ols64_up"),
    ("up", 4, {"fir_up_ols_min": -1, "fir_up_pair": 0}, "fir_ols64_up"),
]


def _signal(dt):
    rng = np.random.default_rng(12289)
    x = rng.standard_normal(N)
    if np.dtype(dt).kind == "c":
        x = (x + 1j * rng.standard_normal(N)) / np.sqrt(2)
    return x.astype(dt)


def _reference(x, what, f):
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if what in ("up", "updn"):
        L, M = f if what == "updn" else (f, 1)
        up = np.zeros(N * L, dtype=xw.dtype)
        up[::L] = L * xw
        return np.convolve(up, B)[:N * L][::M][:N * L // M]
    return np.convolve(xw, B)[:N][::f][:N // f]   # (.filter: f = 1)


def _call(k, xd, what, f, opts):
    """(result, engines launched) of one call on handle k"""
    count = N * f if what == "up" else N * f[0] // f[1] if what == "updn" else N // f
    yd = _ffi.DeviceArray(count, xd.dtype)
    try:
        _ffi.debug_path()
        with contextlib.ExitStack() as st:
            for name, val in opts.items():
                st.enter_context(_ffi.option(name, val))
            if what == "filter":
                k.filter_dev(xd, yd)
            elif what == "updn":
                k.updn_dev(xd, yd, f[0], f[1])
            else:
                (k.up_dev if what == "up" else k.dn_dev)(xd, yd, f)
        return yd.to_host(), _ffi.debug_path()
    finally:
        yd.free()


def _sequence(dt):
    """(calls, tolerance) of a handle of this dtype"""
    return (SEQUENCE64, TOL64) if np.dtype(dt) in (np.dtype(np.float64), np.dtype(np.complex128)) else (SEQUENCE, TOL)


@pytest.fixture(scope="module", params=[np.complex64, np.float32, np.complex128, np.float64], ids=["complex64", "float32", "complex128", "float64"])
def case_all(request):
    """(dtype, x, {(what, factor): float64 reference}): computed once per dtype"""
    x = _signal(request.param)
    return request.param, x, {(w, f): _reference(x, w, f) for w, f in {(w, f) for w, f, _, _ in _sequence(request.param)[0]}}


@pytest.fixture(scope="module", params=[np.complex64, np.float32], ids=["complex64", "float32"])
def case(request):
    """(dtype, x): the signals of the bank"""
    return request.param, _signal(request.param), None


def test_plans_of_one_handle(case_all):
    dt, x, refs = case_all
    sequence, tol = _sequence(dt)
    xd = _ffi.DeviceArray.from_host(x)
    try:
        for cycle in range(2):   # (the second cycle: create / call / destroy works again behind the first handle's destruction)
            k = _ffi.FirKernel(B, _ffi.code_of(dt))
            first = {}
            for step, (what, f, opts, engine) in enumerate(sequence):
                y, path = _call(k, xd, what, f, opts)
                assert path == [engine], (cycle, step, path)
                ref = refs[(what, f)]
                e = np.max(np.abs(y - ref)) / max(np.max(np.abs(y)), np.max(np.abs(ref)))
                print("%s cycle %d step %d %s by %s through %s: max |y - ref| / peak %.3g" % (np.dtype(dt).name, cycle, step, what, f, engine, e))
                assert e <= tol, (cycle, step, e)
                # a handle that makes only this call computes the same bytes ...
                fresh = _ffi.FirKernel(B, _ffi.code_of(dt))
                y1, path1 = _call(fresh, xd, what, f, opts)
                fresh._fin()
                assert path1 == [engine] and y.tobytes() == y1.tobytes(), (cycle, step)
                # ... and so did this handle when it first made it
                key = (what, f, engine, tuple(sorted(opts.items())))
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


# ---- the IIR handles: what they own is tables per chunk length and per slot, and buffers that grow ----------------------------------------
# (label, design, creation options, [(what, factor, n, options, engines)]).  The engines are the IIR engines the call's path names, in order
# (the resamplers and converters around them are left out; a handle in groups names one per group).  All handles are float32 and alive together; the references are
# scipy.signal.sosfilt in float64 and the tolerance is the float32 contract above.
N_SHORT = 4096
UP_T64 = 344   # n L > 2^22 outputs: the first factor whose two-pass chunk is 64 samples, not 32 (iir_scan_plan.hpp: scan_geometry)
IIR_HANDLES = [
    ("e5", "e5", {}, [
        ("filter", 1, N, {"iir_par": 0}, "iir_scan"),          # the cascade scan: tables of 32-sample chunks
        ("up", UP_T64, N, {"iir_par": 0}, "iir_scan"),         # ... of 64-sample chunks: every table of the plan rewritten, G grown
        ("filter", 1, N, {"iir_par": 0}, "iir_scan"),          # ... and back
        ("filter", 1, N, {}, "iir_par"),                       # the parallel form: table slot 0 (128-sample chunks)
        ("dn", 2, N, {}, "iir_par"),                           # slot 4 (96-sample chunks)
        ("up", 8, N, {}, "iir_par"),                           # slot 4 and the jump table of L = 8
        ("up", 12, N, {}, "iir_par"),                          # a second jump table
        ("up", 8, N, {}, "iir_par"),                           # the first found again
        ("filter", 1, N, {}, "iir_par"),
        ("dn", 2, N, {}, "iir_par"),
        ("filter", 1, N, {"iir_par": 0}, "iir_scan"),
    ]),
    ("s65", "s65", {"iir_seq": 2}, [                           # 65 sections as the reference's recursion: two passes meet in a buffer of the handle
        ("filter", 1, N_SHORT, {}, "iir_seq"),
        ("filter", 1, N, {}, "iir_seq"),                       # ... which grows
        ("filter", 1, N_SHORT, {}, "iir_seq"),
    ]),
    ("b16", "b16", {}, [                                       # a plain cascade that stays in float32: groups of 8 + 8 (the parallel form takes one)
        ("filter", 1, N, {}, "iir_scan iir_par"),
        ("dn", 3, N_SHORT, {}, "iir_scan iir_par"),            # the full-rate signal between the groups: a buffer of the handle
        ("dn", 3, N, {}, "iir_scan iir_par"),                  # ... which grows
    ]),
    ("c13", "c13", {}, [                                       # 13 sections no float32 boundary is safe for: widened, the float64 twin, narrowed
        ("filter", 1, N_SHORT, {}, "iir_par"),
        ("filter", 1, N, {}, "iir_par"),                       # the widened copy grows
        ("dn", 3, N, {}, "iir_par"),                           # the twin's kept outputs: a second buffer
    ]),
]
_IIR_ENGINES = ("iir_scan", "iir_fused", "iir_par", "iir_par_v32", "iir_seq")


def _iir_designs():
    signal = pytest.importorskip("scipy.signal")
    return {
        "e5": signal.ellip(10, 0.4, 70, 0.27, output="sos"),
        "s65": np.vstack([signal.butter(2, 0.3 + 0.005 * k, output="sos") for k in range(65)]),
        "b16": signal.butter(32, 0.3, output="sos"),
        "c13": signal.cheby1(26, 0.5, 0.3, output="sos"),
    }


@pytest.fixture(scope="module")
def iir_case():
    """(x, designs, {(design, what, factor, n): float64 reference}): computed once"""
    signal = pytest.importorskip("scipy.signal")
    x = _signal(np.float32)
    designs = _iir_designs()
    refs = {}
    for _, d, _, calls in IIR_HANDLES:
        for what, f, n, _, _ in calls:
            if (d, what, f, n) in refs:
                continue
            xw = x[:n].astype(np.float64)
            if what == "up":
                up = np.zeros(n * f)
                up[::f] = f * xw
                xw = up
            y = signal.sosfilt(designs[d], xw)
            refs[(d, what, f, n)] = y[::f][:n // f] if what == "dn" else y
    return x, designs, refs


def _iir_call(k, xd, what, f, n, opts):
    count = n * f if what == "up" else n // f
    yd = _ffi.DeviceArray(count, xd.dtype)
    try:
        _ffi.debug_path()
        with contextlib.ExitStack() as st:
            for name, val in opts.items():
                st.enter_context(_ffi.option(name, val))
            if what == "filter":
                k.filter_dev(xd, yd, n=n)
            else:
                (k.up_dev if what == "up" else k.dn_dev)(xd, yd, f, n=n)
        return yd.to_host(), [p for p in _ffi.debug_path() if p in _IIR_ENGINES]
    finally:
        yd.free()


def _iir_handle(design, opts):
    with contextlib.ExitStack() as st:
        for name, val in opts.items():
            st.enter_context(_ffi.option(name, val))
        return _ffi.IirKernel(_ffi.code_of(np.float32), sos=design)


def test_iir_plans_of_one_handle(iir_case):
    x, designs, refs = iir_case
    xd = _ffi.DeviceArray.from_host(x)
    try:
        for cycle in range(2):   # (the second cycle: create / call / destroy works again behind the first handles' destruction)
            handles = {label: _iir_handle(designs[d], copts) for label, d, copts, _ in IIR_HANDLES}
            assert handles["s65"].sequential and not handles["c13"].sequential and not handles["b16"].sequential
            first = {}
            for label, d, copts, calls in IIR_HANDLES:
                for step, (what, f, n, opts, engine) in enumerate(calls):
                    y, path = _iir_call(handles[label], xd, what, f, n, opts)
                    assert path and sorted(set(path), key=path.index) == engine.split(), (cycle, label, step, path)
                    ref = refs[(d, what, f, n)]
                    e = np.max(np.abs(y - ref)) / max(np.max(np.abs(y)), np.max(np.abs(ref)))
                    print("%s cycle %d step %d %s by %d of %d through %s: max |y - ref| / peak %.3g" % (label, cycle, step, what, f, n, engine, e))
                    assert e <= TOL, (cycle, label, step, e)
                    # a handle that makes only this call computes the same bytes ...
                    fresh = _iir_handle(designs[d], copts)
                    y1, path1 = _iir_call(fresh, xd, what, f, n, opts)
                    fresh._fin()
                    assert path1 == path and y.tobytes() == y1.tobytes(), (cycle, label, step)
                    # ... and so did this handle when it first made it
                    key = (label, what, f, n, engine, tuple(sorted(opts.items())))
                    assert first.setdefault(key, y).tobytes() == y.tobytes(), (cycle, label, step)
            for k in handles.values():
                k._fin()
    finally:
        xd.free()
