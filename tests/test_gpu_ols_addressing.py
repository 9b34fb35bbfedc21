"""The whole-tile loads and stores of the overlap-save kernels address memory as a uniform 64-bit base per 512-sample block plus one 32-bit
byte offset per lane (csrc/fir_ols.hip: ScalarBase), and the odd column's pass-1 twiddle is one packed product (csrc/ols_core.hpp: mul_w8192).

What can go wrong is the base of a block, the block-to-store mapping of a copy of the stores (one copy per a0 = overlap / 512) and the
cache-policy copy of the loads (one per number of kept blocks), so the shapes are the smallest that drive them: complex64 at 300, 1024, 2049
and 4097 taps (a0 = 1, 2, 5, 8), each at n = V + 5 (one full tile and a ragged one), 3 V (interior tiles only) and 3 V - 1, with Ntaps - 1
samples of history and with none; 1024 taps with x and y 8, 24 and 4088 bytes behind a 4 KiB boundary (the base is no longer block-aligned,
the samples still are); float32 at 1024 taps (two real tiles per complex tile) at 2 V + 5 and 4 V; .dn(x, 4) and .up(x, 4) at 1024 taps and
three tiles; 1024 taps under every value of ols_keep_overlap; and one signal long enough that every workgroup walks a second tile, which is
what drives the copies of the loads inside the tile loop (the prefetch) rather than the one in front of it.

Every case runs twice and must give the same bytes, and is compared with the oracle at 1e-6 of the reference's peak (bench.PARITY_TOL; the
kernel's own error is 2 - 3e-7, float32 butterflies against a float64 sum)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sk_dsp_comm_amd import _ffi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

TOL = 1e-6


def lowpass(ntaps, cutoff):
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = cutoff * np.sinc(cutoff * m) * np.hamming(ntaps)
    return h / np.sum(h)


def tile_outputs(ntaps):
    ov = max(512, -(-(ntaps - 1) // 512) * 512)
    return 8192 - ov


def length_of(ntaps, which):
    V = tile_outputs(ntaps)
    return {"V+5": V + 5, "3V": 3 * V, "3V-1": 3 * V - 1, "2V+5": 2 * V + 5, "4V": 4 * V}[which]


def rel_peak(y, ref):
    return float(np.max(np.abs(y.astype(ref.dtype) - ref)) / np.max(np.abs(ref)))


def noise(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(dtype)
    return rng.standard_normal(n).astype(dtype)


def twice(call, yd, n_out, want_path):
    """call() two times -> the output of the first run; the second must be the same bytes."""
    outs = []
    for _ in range(2):
        check = yd.dtype.type(7)   # (a run that stores nothing is seen)
        yd.write(np.full(min(n_out, 64), check, yd.dtype))
        _ffi.debug_path()
        call()
        _ffi.sync()
        path = _ffi.debug_path()
        assert want_path in path, path
        outs.append(yd.to_host(0, n_out))
    assert outs[0].tobytes() == outs[1].tobytes(), "two runs differ"
    return outs[0]


def check_filter(ntaps, n, hist, dtype=np.complex64, x_shift=0, y_shift=0, label=""):
    """.filter through fir_ols; x_shift / y_shift: bytes that x[0] / y[0] lie behind a 4 KiB boundary (0: wherever the allocation puts them)."""
    _ffi.init(0)
    b = lowpass(ntaps, 0.2)
    k = _ffi.FirKernel(b, _ffi.code_of(dtype))
    k.set_algo(_ffi.FIR_OLS)
    P = ntaps - 1
    esz = np.dtype(dtype).itemsize
    slack = 4096 // esz
    xbuf = _ffi.DeviceArray(n + slack, dtype, headroom=P + slack)
    ybuf = _ffi.DeviceArray(n + slack, dtype)
    sx = ((x_shift - xbuf.ptr) % 4096) // esz if x_shift else 0   # samples into the buffer at which x[0] has the wanted address
    sy = ((y_shift - ybuf.ptr) % 4096) // esz if y_shift else 0
    if x_shift:
        assert (xbuf.ptr + sx * esz) % 4096 == x_shift and (ybuf.ptr + sy * esz) % 4096 == y_shift
    x = noise(n, dtype, ntaps + n)
    h = noise(P, dtype, ntaps) if hist else np.zeros(0, dtype)
    xbuf.write(x, at=sx)
    if hist:
        xbuf.write(h, at=sx - P)
    xd, yd = xbuf.window(sx, n), ybuf.window(sy, n)
    y = twice(lambda: k.filter_dev(xd, yd, n, P if hist else 0), yd, n, "fir_ols")
    ref = orc.fir_filter(b, np.concatenate([h, x]))[h.size:]
    e = rel_peak(y, ref)
    print("filter %s taps %d n %d hist %s %s: %.3g" % (np.dtype(dtype).name, ntaps, n, hist, label, e))
    assert e < TOL, (ntaps, n, hist, label, e)


@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("which", ["V+5", "3V", "3V-1"])
@pytest.mark.parametrize("ntaps", [300, 1024, 2049, 4097])
def test_filter_c64(ntaps, which, hist):
    check_filter(ntaps, length_of(ntaps, which), hist)


@pytest.mark.parametrize("shift", [8, 24, 4088])
def test_filter_c64_shifted_base(shift):
    check_filter(1024, length_of(1024, "3V"), True, x_shift=shift, y_shift=shift, label="x, y %d bytes behind a 4 KiB boundary" % shift)


@pytest.mark.parametrize("which", ["2V+5", "4V"])
def test_filter_f32_two_real_tiles(which):
    check_filter(1024, length_of(1024, which), True, dtype=np.float32)


@pytest.mark.parametrize("keep", [0, 1, 2])
def test_filter_c64_keep_overlap(keep):
    with _ffi.option("ols_keep_overlap", keep):
        check_filter(1024, length_of(1024, "3V"), True, label="ols_keep_overlap %d" % keep)


def test_filter_c64_prefetch_copies():
    """Every workgroup walks two tiles and some a third: the x loads inside the tile loop.  Windows at the head, across the boundary between the
    first and the second round and at the tail."""
    _ffi.init(0)
    ntaps, WIN = 1024, 2048
    V = tile_outputs(ntaps)
    grid = 2 * _ffi.device_info()["compute_units"]
    n = (2 * grid + 3) * V - V // 3
    b = lowpass(ntaps, 0.2)
    k = _ffi.FirKernel(b, _ffi.C64)
    k.set_algo(_ffi.FIR_OLS)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=1024).fill_noise(11)
    yd = _ffi.DeviceArray(n, np.complex64)
    y = twice(lambda: k.filter_dev(xd, yd), yd, n, "fir_ols")
    x = xd.to_host()
    P = ntaps - 1
    for s in (0, grid * V - WIN // 2, 2 * grid * V - WIN // 2, n - WIN):
        s = max(s, 0)
        lead = min(P, s)
        ref = orc.fir_filter(b, x[s - lead:s + WIN])[lead:]
        e = rel_peak(y[s:s + WIN], ref)
        print("filter complex64 taps 1024 n %d window %d: %.3g" % (n, s, e))
        assert e < TOL, (s, e)


def test_dn4_three_tiles():
    _ffi.init(0)
    ntaps, M = 1024, 4
    n = 3 * tile_outputs(ntaps)
    b = lowpass(ntaps, 0.2 / M)
    k = _ffi.FirKernel(b, _ffi.C64)
    k.set_algo(_ffi.FIR_OLS)
    x = noise(n, np.complex64, 41)
    xd = _ffi.DeviceArray.from_host(x, headroom=1024)
    yd = _ffi.DeviceArray(n // M, np.complex64)
    y = twice(lambda: k.dn_dev(xd, yd, M), yd, n // M, "fir_ols")
    e = rel_peak(y, orc.fir_dn(b, x, M))
    print("dn4 taps 1024 n %d: %.3g" % (n, e))
    assert e < TOL, e


def test_up4_three_tiles():
    _ffi.init(0)
    ntaps, L = 1024, 4
    n = 3 * tile_outputs(ntaps) // L   # three tiles of the OUTPUT
    b = lowpass(ntaps, 0.2 / L)
    k = _ffi.FirKernel(b, _ffi.C64)
    x = noise(n, np.complex64, 43)
    xd = _ffi.DeviceArray.from_host(x, headroom=1024)
    yd = _ffi.DeviceArray(n * L, np.complex64)
    with _ffi.option("fir_up_rep", 2):   # (the tiles-of-the-output engine wherever it applies, whatever the cost model says of so short a signal)
        y = twice(lambda: k.up_dev(xd, yd, L), yd, n * L, "fir_ols_rep")
    e = rel_peak(y, orc.fir_up(b, x, L))
    print("up4 taps 1024 n %d: %.3g" % (n, e))
    assert e < TOL, e
