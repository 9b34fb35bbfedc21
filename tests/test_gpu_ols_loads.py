"""The cache policy of the overlap-save x loads (option ols_keep_overlap) must not change a value.

load_tile (csrc/fir_ols.hip) requests the sixteen 512-sample blocks of an interior tile with one of three policies: 0 all nontemporal, 1 the blocks
a tile shares with its neighbours ordinary and the rest nontemporal, 2 all ordinary.  Each policy is its own copy of the sixteen loads (one per
number of kept blocks a plan can produce), so every copy is driven here: tap counts 2, 513, 1024, 4097 (a0 = 1, 1, 2, 8 shared blocks), a signal
long enough that some workgroup walks three tiles (first load, prefetch, both kinds of block) with a ragged last tile, with and without history
in front of x, x one sample into its buffer, and x at an address that is no multiple of the sample size (the element-wise edge path for every
tile).  Per case and option, 2048-sample windows at the head, across two tile boundaries and at the tail are compared with the oracle
(1e-6 of the window's peak: bench.PARITY_TOL), and the whole outputs of the three options must be the same bits.  .dn(x, 4) and .up(x, 4) at
1024 taps run through the same checks on one size each."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sk_dsp_comm_amd import _ffi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

TOL = 1e-6
WIN = 2048
OPTIONS = (0, 1, 2)


def lowpass(ntaps, cutoff):
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = cutoff * np.sinc(cutoff * m) * np.hamming(ntaps)
    return h / np.sum(h)


def tile_outputs(ntaps):
    ov = max(512, -(-(ntaps - 1) // 512) * 512)
    return 8192 - ov


def walk_grid():
    """Workgroups of the persistent launch (fir_ols_launch): two per CU less the reserved slots."""
    _ffi.init(0)
    grid = 2 * _ffi.device_info()["compute_units"]
    reserve = _ffi.get_option("ols_reserve")
    if reserve > 0 and grid >= 4 * reserve:
        grid -= reserve
    return grid


def samples_for(V, grid):
    return (2 * grid + 3) * V - V // 3   # 2 grid + 3 tiles, the last one ragged


class _Shifted:
    """x of a DeviceArray seen `nbytes` further on (what a caller's pointer into a larger buffer looks like)."""

    def __init__(self, base, nbytes, n):
        self.ptr, self.n, self.dtype, self._owner = base.ptr + nbytes, n, base.dtype, base


def rel_peak(y, ref):
    return float(np.max(np.abs(y.astype(np.complex128) - ref)) / np.max(np.abs(ref)))


def run_options(call, yd, n_out):
    """call() under each option value -> the three outputs on the host."""
    outs = []
    for o in OPTIONS:
        with _ffi.option("ols_keep_overlap", o):
            _ffi.debug_path()
            call()
            _ffi.sync()
            path = _ffi.debug_path()
        outs.append((path, yd.to_host(0, n_out)))
    return outs


FILTER_CASES = [(ntaps, hist, "none") for ntaps in (2, 513, 1024, 4097) for hist in (False, True)] + [(1024, False, "sample"), (1024, False, "bytes4")]


@pytest.mark.parametrize("ntaps,hist,shift", FILTER_CASES)
def test_filter_load_policies(ntaps, hist, shift):
    grid = walk_grid()
    V = tile_outputs(ntaps)
    n = samples_for(V, grid)
    b = lowpass(ntaps, 0.2)
    k = _ffi.FirKernel(b, _ffi.C64)
    k.set_algo(_ffi.FIR_OLS)
    P = ntaps - 1
    buf = _ffi.DeviceArray(n + 2, np.complex64, headroom=4096).fill_noise(3)
    h = None
    if hist:
        rng = np.random.default_rng(ntaps)
        h = ((rng.standard_normal(P) + 1j * rng.standard_normal(P)) / np.sqrt(2)).astype(np.complex64)
        buf.write(h, at=-P)
    xd = {"none": buf.window(0, n), "sample": buf.window(1, n), "bytes4": _Shifted(buf, 4, n)}[shift]
    yd = _ffi.DeviceArray(n, np.complex64)
    x_all = buf.to_host(0, n + 2)
    if shift == "bytes4":   # the samples as the kernel sees them: (im k, re k+1)
        x = x_all.view(np.float32)[1:2 * n + 1].copy().view(np.complex64)
    else:
        x = x_all[1:n + 1] if shift == "sample" else x_all[:n]
    outs = run_options(lambda: k.filter_dev(xd, yd, n, P if hist else 0), yd, n)
    xe = np.concatenate([h if hist else np.zeros(P, np.complex64), x])   # x[-P ..] as the call defines it
    starts = [0, V - WIN // 2, (grid + 1) * V - WIN // 2, n - WIN]
    for s in starts:
        ref = orc.fir_filter(b, xe[P + s:P + s + WIN], hist=xe[s:P + s])
        for o, (path, y) in zip(OPTIONS, outs):
            assert "fir_ols" in path, path
            e = rel_peak(y[s:s + WIN], ref)
            print("taps %d hist %s shift %s option %d window %d: %.3g" % (ntaps, hist, shift, o, s, e))
            assert e < TOL, (ntaps, hist, shift, o, s, e)
    for o, (_, y) in zip(OPTIONS[1:], outs[1:]):
        assert np.array_equal(y.view(np.uint32), outs[0][1].view(np.uint32)), "option %d differs from option 0" % o


def test_dn4_load_policies():
    grid = walk_grid()
    ntaps, M = 1024, 4
    V = tile_outputs(ntaps)
    n = samples_for(V, grid)
    b = lowpass(ntaps, 0.2 / M)
    k = _ffi.FirKernel(b, _ffi.C64)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=4096).fill_noise(5)
    yd = _ffi.DeviceArray(n // M, np.complex64)
    x = xd.to_host()
    outs = run_options(lambda: k.dn_dev(xd, yd, M), yd, n // M)
    P = ntaps - 1
    n_out = n // M
    for j in [0, V // M - WIN // 2, (grid + 1) * V // M - WIN // 2, n_out - WIN]:   # windows of the OUTPUT; tiles are V inputs
        s = j * M
        ref = orc.fir_filter(b, x[s:s + WIN * M], hist=x[max(0, s - P):s] if s else None)[::M]
        for o, (path, y) in zip(OPTIONS, outs):
            assert "fir_ols" in path, path
            e = rel_peak(y[j:j + WIN], ref)
            print("dn4 option %d window %d: %.3g" % (o, j, e))
            assert e < TOL, (o, j, e)
    for o, (_, y) in zip(OPTIONS[1:], outs[1:]):
        assert np.array_equal(y.view(np.uint32), outs[0][1].view(np.uint32)), "option %d differs from option 0" % o


@pytest.mark.parametrize("engine", ["default", "walk"])
def test_up4_load_policies(engine):
    """default: what AUTO takes (tiles of the output, whose loads are nontemporal whatever the option says); walk: the walk over (tile, phase)
    pairs, which shares load_tile with .filter."""
    grid = walk_grid()
    ntaps, L = 1024, 4
    b = lowpass(ntaps, 0.2 / L)
    if engine == "walk":
        V = tile_outputs(ntaps // L)           # tiles of the INPUT, four phases of 256 taps each
        n = samples_for(V, grid) // L          # (2 grid + 3) / 4 input tiles, four (tile, phase) pairs each
        opts = [("fir_up_rep", 0), ("fir_up4k", 0), ("fir_up_ols_min", -1)]   # (no other engine, no cost model)
    else:
        V = tile_outputs(ntaps)                # tiles of the OUTPUT
        n = samples_for(V, grid) // L
        opts = []
    k = _ffi.FirKernel(b, _ffi.C64)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=4096).fill_noise(9)
    yd = _ffi.DeviceArray(n * L, np.complex64)
    x = xd.to_host()
    old = [(name, _ffi.set_option(name, v)) for name, v in opts]
    try:
        outs = run_options(lambda: k.up_dev(xd, yd, L), yd, n * L)
    finally:
        for name, v in old:
            _ffi.set_option(name, v)
    H = (ntaps - 1 + L - 1) // L   # input samples in front of a window that reach into it
    step = V * L if engine == "walk" else V   # outputs per tile
    second = (grid // L + 1) * step if engine == "walk" else (grid + 1) * step   # a tile of some workgroup's second round
    for s in [0, step - WIN // 2, second - WIN // 2, n * L - WIN]:
        s -= s % L
        i0 = s // L
        lead = min(H, i0)
        ref = orc.fir_up(b, x[i0 - lead:i0 + WIN // L], L)[lead * L:]
        for o, (path, y) in zip(OPTIONS, outs):
            if engine == "walk":
                assert "fir_ols_up" in path, path
            e = rel_peak(y[s:s + WIN], ref)
            print("up4 %s %s option %d window %d: %.3g" % (engine, path, o, s, e))
            assert e < TOL, (engine, o, s, e)
    for o, (_, y) in zip(OPTIONS[1:], outs[1:]):
        assert np.array_equal(y.view(np.uint32), outs[0][1].view(np.uint32)), "option %d differs from option 0" % o
