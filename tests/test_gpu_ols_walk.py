"""The two walks of the overlap-save tile kernel (csrc/fir_ols.hip: ols_tile_kernel; csrc/ols_walk.hpp): option ols_walk = 0 deals every
workgroup its tiles, 2 lets the workgroups of every form of the kernel draw them from per-XCD ranges, 1 (the default) those of the plain
filter.  Which workgroup computes a tile does not enter the tile's arithmetic, so all must give THE SAME BYTES.

Every call runs under the three values, twice each: 300 and 1024 taps, complex64 and float32, .filter and .dn(x, 3) (the decimating store of
the same kernel), at n = 3 V + 100 (fewer tiles than XCD ranges can fill: empty ranges, workgroups that draw nothing of their own), grid V + 1
(one tile per workgroup and one more) and (2 grid + 3) V + 17 (every workgroup draws in the tile loop, the ranges end at different times),
with V the outputs of a tile and grid the launch's workgroups.  One call has a NaN in an interior tile: the poisoned-tile replay goes by walk
step, and the claimed walk has to remember which tile each step drew.

Checks: the two runs of a walk give the same bytes, the two walks give the same bytes, and each meets the oracle at 1e-6 of the reference's
peak (bench.PARITY_TOL; the kernel's own error is 2 - 3e-7) on a window at the head, one in the interior and one at the tail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sk_dsp_comm_amd import _ffi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

TOL = 1e-6
WIN = 2048   # outputs per compared window


def lowpass(ntaps, cutoff):
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = cutoff * np.sinc(cutoff * m) * np.hamming(ntaps)
    return h / np.sum(h)


def tile_outputs(ntaps):
    ov = max(512, -(-(ntaps - 1) // 512) * 512)
    return 8192 - ov


def launch_grid():
    grid = 2 * _ffi.device_info()["compute_units"]
    reserve = _ffi.get_option("ols_reserve")
    return grid - reserve if reserve > 0 and grid >= 4 * reserve else grid


def length_of(ntaps, which):
    V, grid = tile_outputs(ntaps), launch_grid()
    return {"3V+100": 3 * V + 100, "gridV+1": grid * V + 1, "(2grid+3)V+17": (2 * grid + 3) * V + 17}[which]


def rel_peak(y, ref):
    return float(np.max(np.abs(y.astype(ref.dtype) - ref)) / np.max(np.abs(ref)))


def run_walks(call, yd, n_out):
    """call() twice under each value of ols_walk -> the output; all runs must be the same bytes.  (0: dealt.  2: every form of the kernel claimed.
    1, the default: the plain filter claimed, the decimating store dealt.)"""
    outs = {}
    for walk in (0, 1, 2):
        with _ffi.option("ols_walk", walk):
            for rep in range(2):
                yd.write(np.full(min(n_out, 64), yd.dtype.type(7), yd.dtype))   # (a run that stores nothing is seen)
                _ffi.debug_path()
                call()
                _ffi.sync()
                path = _ffi.debug_path()
                assert "fir_ols" in path, path
                y = yd.to_host(0, n_out)
                if rep == 0:
                    outs[walk] = y
                else:
                    assert outs[walk].tobytes() == y.tobytes(), "walk %d: two runs differ" % walk
    assert outs[0].tobytes() == outs[2].tobytes(), "the dealt and the claimed walk differ"
    assert outs[0].tobytes() == outs[1].tobytes(), "the default walk differs from the dealt one"
    return outs[0]


def windows_of(n_out):
    return sorted({0, max(0, n_out // 2 - WIN // 2), max(0, n_out - WIN)})


def check_against_oracle(y, x, b, M, label):
    """Output windows against the oracle's filter over the samples they depend on (output m of .dn is full-rate output m M)."""
    P = b.size - 1
    for m0 in windows_of(y.size):
        m1 = min(y.size, m0 + WIN)
        s0, s1 = m0 * M, (m1 - 1) * M + 1            # the full-rate outputs behind the window
        lead = min(P, s0)
        ref = orc.fir_filter(b, x[s0 - lead:s1])[lead:][::M]
        e = rel_peak(y[m0:m1], ref)
        print("%s window %d: %.3g" % (label, m0, e))
        assert e < TOL, (label, m0, e)


@pytest.mark.parametrize("call", ["filter", "dn3"])
@pytest.mark.parametrize("which", ["3V+100", "gridV+1", "(2grid+3)V+17"])
@pytest.mark.parametrize("dtype", [np.complex64, np.float32])
@pytest.mark.parametrize("ntaps", [300, 1024])
def test_both_walks(ntaps, dtype, which, call):
    _ffi.init(0)
    M = 3 if call == "dn3" else 1
    n = length_of(ntaps, which)
    b = lowpass(ntaps, 0.2 / M)
    k = _ffi.FirKernel(b, _ffi.code_of(dtype))
    k.set_algo(_ffi.FIR_OLS)
    xd = _ffi.DeviceArray(n, dtype, headroom=ntaps).fill_noise(ntaps + M)
    n_out = n // M
    yd = _ffi.DeviceArray(n_out, dtype)
    with _ffi.option("fir_dn4k", 0):   # (.dn through the decimating store of ols_tile_kernel, whatever the cost model says of the shape)
        y = run_walks((lambda: k.dn_dev(xd, yd, M)) if M > 1 else (lambda: k.filter_dev(xd, yd)), yd, n_out)
    check_against_oracle(y, xd.to_host(), b, M, "%s %s taps %d n %d" % (call, np.dtype(dtype).name, ntaps, n))


def test_both_walks_poisoned_interior_tile():
    """A NaN in the second tile a workgroup walks: the kernel notes the STEP and recomputes that step's tile behind its loop by the reference's
    own sum, which confines the NaN to the Ntaps outputs that multiply it."""
    _ffi.init(0)
    ntaps = 1024
    V, grid = tile_outputs(ntaps), launch_grid()
    n = (2 * grid + 3) * V + 17
    b = lowpass(ntaps, 0.2)
    k = _ffi.FirKernel(b, _ffi.C64)
    k.set_algo(_ffi.FIR_OLS)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=ntaps).fill_noise(5)
    p = (grid + 5) * V + 1234   # inside tile grid + 5, away from its edges
    xd.write(np.array([np.nan + 0j], np.complex64), at=p)
    yd = _ffi.DeviceArray(n, np.complex64)
    y = run_walks(lambda: k.filter_dev(xd, yd), yd, n)
    bad = np.flatnonzero(~np.isfinite(y))
    assert bad.size == ntaps and bad[0] == p and bad[-1] == p + ntaps - 1, (bad.size, bad[:1], bad[-1:], p)
    x = xd.to_host()
    for s in (p - WIN, p + ntaps):   # the finite outputs of the poisoned tile, on both sides
        ref = orc.fir_filter(b, x[s - (ntaps - 1):s + WIN])[ntaps - 1:]
        e = rel_peak(y[s:s + WIN], ref)
        print("poisoned tile, window %d: %.3g" % (s, e))
        assert e < TOL, (s, e)
