"""Carrier phase tracking over frame sets on the GPU (csrc/carrier.hip): the device against the NumPy host forms bit for bit, across lane masks,
partial waves, tile edges, strided reads and strided outputs; every subset of the outputs inside guard bands; the input window alone is read; the
golden cases of the reference within the bound of tests/test_carrier_cpu.py; the impairment kernel; and one BER loop end to end.  DESIGN.md 4.22."""
import json
import os

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dcm, sigsys as ss, synchronization as sync
from conftest import ROOT
from _pads import loud

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "g27_carrier.npz"))
CASES = json.loads(str(G["cases"]))
NAMES = _ffi.CAR_OUTPUTS
T = 8                                    # the kernel's tile length in symbols (tests/test_carrier_cpu.py pins it to the plan)
ROWS, SIZES, WINDOWS = (1, 63, 64, 65, 130), (0, 1, T - 1, T, T + 1, 3 * T + 5), ((0, 1), (5, 4), (3, 7))
PAD = GUARD = 40
TWO_PI = 2 * np.pi


@pytest.fixture(scope="module", autouse=True)
def _device():
    _ffi.init(0)


def symbols(rng, nrow, n, mod_type, M, dt=np.complex128, sigma=0.05):
    if mod_type == "MQAM":
        x_m = 1 if M == 2 else int(round(np.sqrt(M))) - 1
        s = (2 * rng.integers(0, x_m + 1, (nrow, n)) - x_m) + 1j * (2 * rng.integers(0, x_m + 1, (nrow, n)) - x_m)
    elif M == 4:
        s = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (nrow, n))))
    else:
        s = np.exp(1j * 2 * np.pi * rng.integers(0, M, (nrow, n)) / M)
    w = sigma * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))
    phase = 0.2 + 2 * np.pi * 1e-3 * np.arange(n)[None, :] + 0.1 * np.arange(nrow)[:, None]
    return ((s + w) * np.exp(1j * phase)).astype(dt)


def fill_of(kind, count, dt, first=0):
    if kind == "zeros":
        return np.zeros(count, dtype=dt)
    if kind == "nan":
        return np.full(count, np.nan + 1j * np.nan).astype(dt)
    return loud(count, dt, first)


def dev_rows(sym, mod_type, M, BnTs, type=0, open_loop=False, start=0, step=1, outputs=NAMES, fill="loud", x_extra=0, y_extra=0):
    """DD_carrier_sync_rows' kernels on device buffers laid out by the test: the symbols of `sym` sit at start + k step of rows x_stride apart, every
    other element of the input buffer -- pads in front and behind, the gaps between symbols and between rows -- holds `fill`.  The outputs lie
    y_stride apart between guard bands of loud values; what the call must not write is checked here.  Returns (selected outputs, MQAM scales)."""
    fam = _ffi.carrier_family(mod_type)
    nrow, n = sym.shape
    dt = sym.dtype
    span = start + (n - 1) * step + 1 if n else 0
    xs, ys = span + x_extra, n + y_extra
    body = (nrow - 1) * xs + span if nrow and n else 0
    host = fill_of(fill, 2 * PAD + body + 1, dt)
    for r in range(nrow):
        host[PAD + r * xs + start:PAD + r * xs + span:step] = sym[r]
    xbuf = _ffi.DeviceArray.from_host(host)
    xw = xbuf.window(PAD, body + 1)
    k1, k2, gains = _ffi.carrier_gains_rows(BnTs, 0.707, nrow)
    gd = None if gains is None else _ffi.DeviceArray.from_host(gains.reshape(-1))
    rd, r = None, None
    if fam == _ffi.QAM and nrow and n:
        rd = _ffi.DeviceArray(nrow, np.float64)
        _ffi.qam_scale_rows_dev(xw.ptr, xs, start, step, n, nrow, dt, M, rd.ptr)
        r = rd.to_host()
    block = (nrow - 1) * ys + n if nrow and n else 0
    dts = dict(z_prime=dt, a_hat=dt, e_phi=np.float64, theta_h=np.float64)
    marks = {o: loud(2 * GUARD + block + 1, dts[o], 7) for o in outputs}
    bufs = {o: _ffi.DeviceArray.from_host(marks[o]) for o in outputs}
    win = {o: (bufs[o].window(GUARD, block + 1) if o in outputs else None) for o in NAMES}
    _ffi.dd_carrier_rows_dev(xw, n, nrow, fam, M, type, open_loop, k1, k2, win["z_prime"], win["a_hat"], win["e_phi"], win["theta_h"], gd, rd, xs, ys, start, step, dt)
    _ffi.sync()
    got = []
    for o in outputs:
        back = bufs[o].to_host()
        keep = np.ones(back.size, dtype=bool)
        for r_ in range(nrow if n else 0):
            keep[GUARD + r_ * ys:GUARD + r_ * ys + n] = False
        assert np.array_equal(back[keep], marks[o][keep]), "%s: written outside its rows" % o
        got.append(np.stack([back[GUARD + r_ * ys:GUARD + r_ * ys + n] for r_ in range(nrow)]) if nrow else np.zeros((0, n), dtype=dts[o]))
    for d in [xbuf, gd, rd] + list(bufs.values()):
        if d is not None:
            d.free()
    return tuple(got), r


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, name)


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.fixture(scope="module")
def qpsk():
    """one reference for the whole grid: rows are independent and start from rest, so (r rows, n symbols) is a corner of the largest run"""
    sym = symbols(np.random.default_rng(2710), max(ROWS), max(SIZES), "MPSK", 4)
    return sym, sync.DD_carrier_sync_rows_host(sym, 4, 0.05)


@pytest.mark.parametrize("start,step", WINDOWS)
def test_every_row_count_and_length_equals_the_host_form(qpsk, start, step):
    sym, want = qpsk
    for nrow in ROWS:
        for n in SIZES:
            got, _ = dev_rows(sym[:nrow, :n], "MPSK", 4, 0.05, start=start, step=step, x_extra=9, y_extra=3)
            same(got, tuple(w[:nrow, :n] for w in want), (nrow, n, start, step))


PAIRS = [("MPSK", 4, 0), ("MPSK", 2, 1), ("MPSK", 4, 2), ("MQAM", 16, 0), ("MQAM", 4, 1), ("MQAM", 64, 2), ("MPSK", 8, 0), ("MPSK", 8, 1), ("MQAM", 256, 2), ("MQAM", 256, 1)]


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_every_family_and_detector_equals_the_host_form_in_both_dtypes(i):
    mod_type, M, det = PAIRS[i]
    rng = np.random.default_rng(2720 + i)
    start, step = WINDOWS[i % 3]
    for dt in (np.complex128, np.complex64):
        sym = symbols(rng, (65, 130)[i % 2], 3 * T + 5, mod_type, M, dt)
        got, r = dev_rows(sym, mod_type, M, 0.05, det, open_loop=i == 4, start=start, step=step, x_extra=5, y_extra=1)
        want = sync.DD_carrier_sync_rows_host(sym, M, 0.05, mod_type=mod_type, type=det, open_loop=i == 4, r=r)
        same(got, want, (mod_type, M, det, dt))
        assert got[0].dtype == dt and got[2].dtype == np.float64
    if mod_type == "MQAM":          # the public call makes the same scales itself
        pub = sync.DD_carrier_sync_rows(sym, M, 0.05, mod_type=mod_type, type=det, open_loop=i == 4)
        same(pub, want, ("public", mod_type, M, det))


def test_an_unlocked_loop_wraps_exactly():
    sym = symbols(np.random.default_rng(2730), 64, 3 * T + 5, "MQAM", 256)
    got, r = dev_rows(sym, "MQAM", 256, 0.05, 0)
    want = sync.DD_carrier_sync_rows_host(sym, 256, 0.05, mod_type="MQAM", type=0, r=r)
    assert np.max(np.abs(want[2])) > 10
    same(got, want, "unlocked")


def test_every_subset_of_the_outputs_gives_the_same_arrays_and_writes_nothing_else():
    sym = symbols(np.random.default_rng(2731), 65, 2 * T + 3, "MPSK", 8)
    full, _ = dev_rows(sym, "MPSK", 8, 0.05, 1, y_extra=1)
    same(full, sync.DD_carrier_sync_rows_host(sym, 8, 0.05, type=1), "full")
    for mask in range(1, 15):
        outs = tuple(o for j, o in enumerate(NAMES) if mask >> j & 1)
        got, _ = dev_rows(sym, "MPSK", 8, 0.05, 1, outputs=outs, y_extra=1)          # (dev_rows checks the guard bands and the gaps of what it allocates)
        assert len(got) == len(outs) and all(np.array_equal(g, full[NAMES.index(o)]) for g, o in zip(got, outs)), outs
        pub = sync.DD_carrier_sync_rows(sym, 8, 0.05, type=1, outputs=outs)
        assert all(np.array_equal(g, full[NAMES.index(o)]) for g, o in zip(pub, outs)), outs


@pytest.mark.parametrize("mod_type,M,det", [("MPSK", 4, 0), ("MQAM", 16, 2)])
def test_the_device_reads_only_its_input_window(mod_type, M, det):
    """the pads in front of and behind the window, the elements between the symbols and between the rows: zeros, loud values or NaNs there change nothing"""
    sym = symbols(np.random.default_rng(2732), 65, 2 * T + 3, mod_type, M, np.complex64)
    runs = [dev_rows(sym, mod_type, M, 0.05, det, start=5, step=4, fill=f, x_extra=9)[0] for f in ("zeros", "loud", "nan")]
    for other in runs[1:]:
        same(other, runs[0], "fill")
    assert not any(np.any(np.isnan(v)) for v in runs[0])


def test_a_gain_per_row_equals_separate_calls():
    sym = symbols(np.random.default_rng(2733), 3, 3 * T + 5, "MPSK", 4)
    bn = np.array([0.01, 0.05, 0.1])
    got = sync.DD_carrier_sync_rows(sym, 4, bn, type=1)
    same(got, sync.DD_carrier_sync_rows_host(sym, 4, bn, type=1), "per row")
    for r in range(3):
        one = sync.DD_carrier_sync(sym[r], 4, float(bn[r]), type=1)
        assert all(np.array_equal(a[r], b) for a, b in zip(got, one))


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_golden_cases_meet_the_bound_of_the_host_form():
    for c in CASES:
        k = c["key"]
        zp, ah, e, th = sync.DD_carrier_sync(G[k + "_z"], c["M"], c["BnTs"], c["zeta"], c["mod_type"], c["type"], c["open_loop"])
        assert np.array_equal(ah, G[k + "_a_hat"]), k
        bound = 16 * c["S"] + (3e-15 * np.max(np.abs(G[k + "_z_prime"])) if c["mod_type"] == "MQAM" else 0.0)
        d = np.mod(np.abs(th - G[k + "_theta_h"]), TWO_PI)
        errs = (np.max(np.abs(zp - G[k + "_z_prime"])), np.max(np.abs(e - G[k + "_e_phi"])), np.max(np.minimum(d, TWO_PI - d)))
        print("%s: z_prime %.2e e_phi %.2e theta_h %.2e bound %.2e" % ((k,) + errs + (bound,)))
        assert max(errs) <= bound, (k, errs, bound)


# ---------------------------------------------------------------------------------------------------------------- phase_step / time_step
def test_impairment_kernel_equals_the_host_forms():
    rng = np.random.default_rng(2734)
    for dt in (np.complex128, np.complex64):
        z = (rng.standard_normal((5, 301)) + 1j * rng.standard_normal((5, 301))).astype(dt)
        for ns in (1, 4):
            for n_step in (7, -(-301 // ns) - 1, -(-301 // ns), 400):
                p = rng.uniform(-3, 3, 5)
                assert np.array_equal(sync.phase_step_rows(z, ns, p, n_step), sync.phase_step_rows_host(z, ns, p, n_step))
                assert np.array_equal(sync.phase_step_rows(z, ns, 0.4, n_step), sync.phase_step_rows_host(z, ns, 0.4, n_step))
                assert np.array_equal(sync.time_step_rows(z, ns, 3, n_step), sync.time_step_rows_host(z, ns, 3, n_step))
        assert np.array_equal(sync.time_step_rows(z, 4, np.array([0, 1, 2, 3, 9]), 20), sync.time_step_rows_host(z, 4, np.array([0, 1, 2, 3, 9]), 20))
    for s in json.loads(str(G["steps"])):
        fn = sync.phase_step if s["fn"] == "phase_step" else sync.time_step
        assert np.array_equal(fn(G[s["key"] + "_z"], s["ns"], s["step"], s["n_step"]), G[s["key"] + "_y"]), s


def test_impairment_kernel_with_strides_and_guards():
    rng = np.random.default_rng(2735)
    z = (rng.standard_normal((3, 97)) + 1j * rng.standard_normal((3, 97))).astype(np.complex128)
    xs, ys, n_out = 101, 28, 25
    host = loud(2 * PAD + 2 * xs + 97, z.dtype)
    for r in range(3):
        host[PAD + r * xs:PAD + r * xs + 97] = z[r]
    mark = loud(2 * GUARD + 2 * ys + n_out, z.dtype, 3)
    xd, yd = _ffi.DeviceArray.from_host(host), _ffi.DeviceArray.from_host(mark)
    _ffi.phase_step_rows_dev(xd.window(PAD, 2 * xs + 97), yd.window(GUARD, 2 * ys + n_out), 97, 3, 4, 7, np.exp(1j * np.array([0.4]))[0], None, xs, ys)
    back, want = yd.to_host(), sync.phase_step_rows_host(z, 4, 0.4, 7)
    for r in range(3):
        assert np.array_equal(back[GUARD + r * ys:GUARD + r * ys + n_out], want[r])
        mark[GUARD + r * ys:GUARD + r * ys + n_out] = want[r]
    assert np.array_equal(back, mark)
    xd.free(), yd.free()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_ber_loop_with_a_phase_step_counts_the_same_errors_on_both_routes():
    """bits -> mpsk_gray_encode_bb_rows -> the AWGN channel -> matched_filter_rows -> phase_step_rows -> DD_carrier_sync_rows -> mpsk_gray_decode_rows ->
    bit_errors_rows on 65 rows of 200 QPSK symbols: the device route and the host route count the same errors"""
    ns, nrow, nsym = 4, 65, 200
    bits = np.random.default_rng(2736).integers(0, 2, (nrow, 2 * nsym)).astype(np.uint8)
    x_dev, b = dcm.mpsk_gray_encode_bb_rows(bits, ns, 4, 'src')
    x_host, _ = dcm.mpsk_gray_encode_bb_rows_host(bits, ns, 4, 'src')
    assert np.array_equal(x_dev, x_host)
    sigma = float(np.sqrt(ns * np.var(x_host) * 10 ** (-9.0 / 10) / 2))          # Es/N0 = 9 dB, one sigma for the set (cpx_awgn's expression)
    xd, yd = _ffi.DeviceArray.from_host(x_dev.reshape(-1)), _ffi.DeviceArray(x_dev.size, np.complex128)
    _ffi.awgn_rows_dev(xd, yd, x_dev.shape[1], nrow, 2737, g=1.0, sigma=sigma)
    y_dev, y_host = yd.to_host().reshape(x_dev.shape), _ffi.awgn_rows_host(x_host, 1.0, sigma, 2737)
    xd.free(), yd.free()
    assert np.array_equal(y_dev, y_host)
    delay = 2 * 6 * ns
    z_dev, z_host = ss.matched_filter_rows(y_dev, b, delay, 1), ss.matched_filter_rows_host(y_host, b, delay, 1)
    assert np.array_equal(z_dev, z_host)
    p = np.linspace(0.1, 0.5, nrow)
    s_dev, s_host = sync.phase_step_rows(z_dev, ns, p, 60), sync.phase_step_rows_host(z_host, ns, p, 60)
    assert np.array_equal(s_dev, s_host)
    (c_dev,), (c_host,) = sync.DD_carrier_sync_rows(s_dev, 4, 0.05, outputs=("z_prime",)), sync.DD_carrier_sync_rows_host(s_host, 4, 0.05, outputs=("z_prime",))
    assert np.array_equal(c_dev, c_host)
    rx_dev = dcm.mpsk_gray_decode_rows(c_dev, 4)
    rx_host = np.stack([dcm.mpsk_gray_decode_host(row, 4) for row in c_host]).astype(np.uint8)
    n_dev, e_dev = dcm.bit_errors_rows(bits, rx_dev)
    e_host = np.sum(bits[:, :rx_host.shape[1]] != rx_host, axis=1)
    assert n_dev == rx_host.shape[1] and np.array_equal(e_dev, e_host)
    assert 0 < e_dev.sum() < 0.2 * bits.size          # (the loop pulls in and tracks: errors, but far from a coin toss)
