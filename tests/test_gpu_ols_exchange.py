"""The 8192-point overlap-save tile with its inter-pass twiddle reads issued ahead of the exchange writes (csrc/ols_core.hpp: lds_req).

T2 and its transpose live in an LDS object of their own and are read a few entries ahead of the products that use them, in fwd_pass23 /
inv_pass32 (ols_tile_kernel), inv_pass32_fold / inv_pass1_fold (ols_fold_kernel) and fwd_pass23_rep (ols_rep_kernel).  A table read cannot
change a value, so every call must still meet the oracle under the bound tests/test_gpu_parity.py applies to the same call (1e-6, max error
over the reference's peak and relative L2), and every call runs twice: the two results must be the same bytes.  What the second run can show is
an IMAGE read that moved across the barrier or the write it has to follow (the bursts of inv_pass1 / inv_pass1_fold); the tables are constant
behind the set-up barrier, so a table read that moved shows nowhere -- and harms nothing.  Identity with the build before this change is not
a test's business (it needs that build): profiles/r14/README.md records the byte comparison of bench.py --dump-outputs.
The engine note of .dn(x, 4) is "fir_ols" for the folded inverse and for the decimating store alike: that ols_fold_kernel runs rests on the
options set here (fir_dn_fold = 1, fir_dn4k = 0) and on fir_route_dn's rule (csrc/fir_route.hpp) for a forced algorithm, not on the assertion.

Shapes: the smallest that reach an interior tile, both edge tiles and a ragged tail -- 3 V + 100 complex64 samples, 5 V + 17 float32 samples
(two real tiles ride in one complex tile), V the outputs per tile; 300, 1024 and 4097 taps (a0 = 1, 2, 8 overlap blocks).  For .up the
sizes are those of the OUTPUT (the tiles of ols_rep_kernel are tiles of the output)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sk_dsp_comm_amd import _ffi  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from conftest import rel_err  # noqa: E402

TOL32 = 1e-6   # tests/test_gpu_parity.py: float32 / complex64 filtering
TAPS = (300, 1024, 4097)
DTYPES = (np.complex64, np.float32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _ffi.init()
    assert "gfx950" in _ffi.device_info()["name"]
    yield


def tile_outputs(ntaps):
    ov = max(512, -(-(ntaps - 1) // 512) * 512)
    return 8192 - ov


def samples(dt, ntaps):
    V = tile_outputs(ntaps)
    return 3 * V + 100 if dt is np.complex64 else 5 * V + 17


def signal(dt, n, seed):
    rng = np.random.default_rng(seed)
    if dt is np.complex64:
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def taps_of(ntaps, rate=1):
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = (0.2 / rate) * np.sinc((0.2 / rate) * m) * np.hamming(ntaps)
    return h / np.sum(h)


def kernel(b, dt):
    k = _ffi.FirKernel(b, _ffi.code_of(np.dtype(dt)))
    k.set_algo(_ffi.FIR_OLS)
    return k


def twice(call, ref, engine, what, options=()):
    """call() two times under `options`: the engine reached, both results against the oracle, and the same bytes."""
    old = [(name, _ffi.set_option(name, v)) for name, v in options]
    try:
        outs = []
        for _ in range(2):
            _ffi.debug_path()
            y = call()
            path = _ffi.debug_path()
            assert engine in path, (what, path)
            outs.append(np.ascontiguousarray(y))
    finally:
        for name, v in old:
            _ffi.set_option(name, v)
    for y in outs:
        assert y.shape == ref.shape, (what, y.shape, ref.shape)
        e_max, e_l2 = rel_err(y, ref)
        print("%s: max/peak %.3g, rel-L2 %.3g" % (what, e_max, e_l2))
        assert e_max <= TOL32 and e_l2 <= TOL32, (what, e_max, e_l2)
    assert outs[0].tobytes() == outs[1].tobytes(), "%s: two runs of one call differ" % what


@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_filter(dt, ntaps):
    n = samples(dt, ntaps)
    x, b = signal(dt, n, ntaps), taps_of(ntaps)
    k = kernel(b, dt)
    assert k.algo_for(n) == _ffi.FIR_OLS
    twice(lambda: k.filter(x), orc.fir_filter(b, x), "fir_ols", "filter %s %d taps" % (np.dtype(dt).name, ntaps))


@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_filter_with_history(dt, ntaps):
    """x[-P .. -1] in front of the buffer is the filter's past (what the sharded and streaming callers pass)."""
    n, P = samples(dt, ntaps), ntaps - 1
    x, b = signal(dt, n + P, ntaps + 1), taps_of(ntaps)
    k = kernel(b, dt)
    xd = _ffi.DeviceArray.from_host(x[P:], headroom=P)
    hist = np.ascontiguousarray(x[:P])
    _ffi.check(_ffi.load().skdsp_memcpy_h2d(ctypes.c_void_p(xd.ptr - hist.nbytes), ctypes.c_void_p(hist.ctypes.data), hist.nbytes))
    yd = _ffi.DeviceArray(n, dt)

    def call():
        k.filter_dev(xd, yd, n, n_hist=P)
        return yd.to_host()

    twice(call, orc.fir_filter(b, x[P:], hist=hist), "fir_ols", "filter + history %s %d taps" % (np.dtype(dt).name, ntaps))


@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_dn4_folded_inverse(dt, ntaps):
    n = samples(dt, ntaps)
    x, b = signal(dt, n, ntaps + 2), taps_of(ntaps, 4)
    k = kernel(b, dt)
    twice(lambda: k.dn(x, 4), orc.fir_dn(b, x, 4), "fir_ols", "dn4 %s %d taps" % (np.dtype(dt).name, ntaps), [("fir_dn_fold", 1), ("fir_dn4k", 0)])


@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_dn3_decimating_store(dt, ntaps):
    n = samples(dt, ntaps)
    x, b = signal(dt, n, ntaps + 3), taps_of(ntaps, 3)
    k = kernel(b, dt)
    twice(lambda: k.dn(x, 3), orc.fir_dn(b, x, 3), "fir_ols", "dn3 %s %d taps" % (np.dtype(dt).name, ntaps), [("fir_dn4k", 0)])


@pytest.mark.parametrize("L", (4, 12))
@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_up_replicated_spectrum(dt, ntaps, L):
    """L = 4: LF = 4; L = 12: LF = 4 on a grid that is itself zero-stuffed three-fold (rep_lr = 3)."""
    n_in = -(-samples(dt, ntaps) // L)
    x, b = signal(dt, n_in, ntaps + L), taps_of(ntaps, L)
    k = kernel(b, dt)
    twice(lambda: k.up(x, L), orc.fir_up(b, x, L), "fir_ols_rep", "up%d %s %d taps" % (L, np.dtype(dt).name, ntaps), [("fir_up_rep", 2)])
