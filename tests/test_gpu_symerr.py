"""The symbol-error tools on the device (csrc/symerr.hip): lag_corr_dev against an int64 NumPy evaluation (exactly) and against xcorr_host
(1e-12 on the normalised correlation, the project's float64 parity figure: DESIGN.md 4.20), twice with the same bits; sym_count_rows_dev against
its host form exactly, inside guarded buffers, over every mode and rotation; every precondition violation; the public functions against their
host forms and the g25 fixtures, with host and DeviceArray arguments; and one device-resident 16-QAM loop against its host restatement and the
closed-form symbol error probability.  Shapes are the smallest that reach every path: K around the tile (1024 samples), lag windows around the
group (256 lags), more than one partition (K = 65538: 65 tiles), symbol counts around the work item (2048 symbols)."""
import json
import logging
import math
import os

import numpy as np
import pytest

from _pads import loud
from conftest import ROOT
from sk_dsp_comm_amd import _ffi, digitalcom as dc

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "g25_symerr.npz"))
SEP, BPSK, QPSK, XC = (json.loads(str(G[k])) for k in ("sep", "bpsk", "qpsk", "xcorr"))
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
PAD = 4096
FILL = 0xEE


@pytest.fixture(scope="module", autouse=True)
def _device():
    _ffi.init(0)


@pytest.fixture(autouse=True)
def _fresh_path():
    _ffi.debug_path()      # (what earlier calls launched)


def int_stream(rng, n, dt, top=15):
    v = rng.integers(-top, top + 1, n).astype(np.float64)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.integers(-top, top + 1, n)
    return v.astype(dt)


def exact_lag_sums(a, b, lags):
    """int64 evaluation of sum_n a[(n + l) mod K] conj(b[n]): the rows of a sliding window over a doubled stream, times b"""
    K = a.size
    ar, ai, br, bi = (np.rint(v).astype(np.int64) for v in (a.real, a.imag, b.real, b.imag))
    first = int(lags[0]) % K
    span = first + len(lags) - 1 + K
    reps = -(-span // K)
    wr = np.lib.stride_tricks.sliding_window_view(np.tile(ar, reps)[first:span], K)
    wi = np.lib.stride_tricks.sliding_window_view(np.tile(ai, reps)[first:span], K)
    return wr @ br + wi @ bi, wi @ br - wr @ bi


class Guarded:
    """`count` elements of `dt` on the device, `off` elements behind a 256-byte boundary, loud values in front of and behind them"""

    def __init__(self, values, dt, off=0):
        self.dt = np.dtype(dt)
        esz = self.dt.itemsize
        values = np.ascontiguousarray(values, dtype=self.dt).reshape(-1)
        npad = PAD // esz
        host = np.concatenate((loud(npad + off, self.dt), values, loud(npad + 3, self.dt, npad + off + values.size)))
        self.dev = _ffi.device_bytes_of(host)
        self.ptr = self.dev.ptr + (npad + off) * esz

    def free(self):
        self.dev.free()


class GuardedOut:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.dev = _ffi.device_bytes_of(np.full(2 * PAD + nbytes, FILL, dtype=np.uint8))
        self.ptr = self.dev.ptr + PAD

    def read(self, dt):
        raw = self.dev.read()
        assert np.all(raw[:PAD] == FILL) and np.all(raw[PAD + self.nbytes:] == FILL), "bytes outside the result changed"
        return raw[PAD:PAD + self.nbytes].view(dt).copy()

    def free(self):
        self.dev.free()


def run_lag(a, b, n_lags, quant=0, off=0):
    nl, l0 = _ffi.lag_corr_len(a.size, n_lags)
    ga, gb, out = Guarded(a, a.dtype, off), Guarded(b, b.dtype, off), GuardedOut(16 * (nl + 1))
    try:
        _ffi.lag_corr_dev(ga.ptr, gb.ptr, a.size, n_lags, out.ptr, out.ptr + 16 * nl, quant, a.dtype, b.dtype)
        assert _ffi.debug_path() == (["lagcorr"] if nl else [])
        res = out.read(np.complex128)
    finally:
        for g in (ga, gb, out):
            g.free()
    return res[:nl], l0 + np.arange(nl), res[nl].real, res[nl].imag


# ---------------------------------------------------------------------------------------------------------------- lag_corr_dev
@pytest.mark.parametrize("n", (2, 3, 64, 1022, 1023, 4098, 65538))
def test_lag_corr_dev_is_exact_on_integers_and_meets_the_float64_bound(n):
    rng = np.random.default_rng(2510 + n)
    K = 2 * (n // 2)
    windows = [0, 1, 7, 300, 1024] + ([K // 2, 10 ** 6] if K <= 1022 else [])
    widest = min(max(windows), K // 2)
    for i, n_lags in enumerate(windows):
        adt, bdt = DTYPES[(i + n) % 4], DTYPES[(i + n // 2 + 1) % 4]
        a, b = int_stream(rng, n, adt), int_stream(rng, n, bdt)
        R, lags, E1, E2 = run_lag(a, b, n_lags, off=i % 3 if adt != np.complex128 and bdt != np.complex128 else 0)
        assert lags.size == min(2 * n_lags + 1, K) and lags[0] == -min(n_lags, K // 2)
        ac, bc = a[:K].astype(np.complex128), b[:K].astype(np.complex128)
        if K < 65538 or n_lags == widest or n_lags == 7:                   # (the widest window of the long stream costs a second of int64 NumPy)
            wre, wim = exact_lag_sums(ac, bc, lags)
            assert np.array_equal(R.real, wre) and np.array_equal(R.imag, wim), (n, n_lags)
        assert E1 == np.sum(ac.real ** 2 + ac.imag ** 2) and E2 == np.sum(bc.real ** 2 + bc.imag ** 2)
        # float streams: the same shapes, against the reference-form host FFT; two runs give the same bits
        fa = (a * 0.173 + 0.01 * int_stream(rng, n, adt)).astype(adt)
        fb = (b * 0.219 - 0.02 * int_stream(rng, n, bdt)).astype(bdt)
        R1, _, e1, e2 = run_lag(fa, fb, n_lags)
        R2, _, f1, f2 = run_lag(fa, fb, n_lags)
        assert R1.tobytes() == R2.tobytes() and (e1, e2) == (f1, f2)
        want, k = dc.xcorr_host(fa, fb, n_lags)
        err = float(np.max(np.abs(R1 / np.sqrt(e1 * e2) - want)))
        print("lag_corr_dev", n, n_lags, np.dtype(adt).name, np.dtype(bdt).name, err)
        assert np.array_equal(k, lags) and err <= 1e-12


def test_lag_corr_dev_quantises_at_the_load():
    rng = np.random.default_rng(2511)
    for M, dt in ((2, np.complex64), (4, np.complex128), (8, np.complex64), (16, np.complex128)):
        tx = ((2 * rng.integers(0, M, 4098) - (M - 1)) + 1j * (2 * rng.integers(0, M, 4098) - (M - 1))).astype(np.complex128)
        soft = (np.roll(tx, 9) / (M - 1) + 0.3 * (rng.standard_normal(4098) + 1j * rng.standard_normal(4098))).astype(dt)
        R, lags, E1, E2 = run_lag(soft, tx, 300, quant=M)
        q = _ffi.qam_quantise_host(soft, M)
        wre, wim = exact_lag_sums(q, tx, lags)
        assert np.array_equal(R.real, wre) and np.array_equal(R.imag, wim) and E1 == np.sum(q.real ** 2 + q.imag ** 2)
        assert lags[np.argmax(R.real)] == 9


def test_host_pointer_lag_corr_equals_the_device_form():
    rng = np.random.default_rng(2512)
    for n, n_lags, adt, bdt, M in ((4099, 300, np.complex64, np.float64, 0), (1022, 10 ** 6, np.float32, np.complex128, 0), (3000, 64, np.complex128, np.complex128, 8)):
        a = (int_stream(rng, n, adt) / (15.0 if M else 1.0)).astype(adt)
        b = int_stream(rng, n, bdt)
        R, lags, E1, E2 = _ffi.lag_corr(a, b, n_lags, M)
        assert _ffi.debug_path() == ["lagcorr"]
        Rd, ld, e1, e2 = run_lag(a, b, n_lags, M)
        assert R.tobytes() == Rd.tobytes() and np.array_equal(lags, ld) and (E1, E2) == (e1, e2)
        Rh, lh, h1, h2 = _ffi.lag_corr_host(a, b, n_lags, M)
        assert np.array_equal(lags, lh) and np.max(np.abs(R - Rh)) <= 1e-12 * np.sqrt(h1 * h2) and abs(E1 - h1) <= 1e-12 * h1 and abs(E2 - h2) <= 1e-12 * h2
    R, lags, E1, E2 = _ffi.lag_corr(np.ones(1), np.ones(1), 5)
    assert R.size == 0 and lags.size == 0 and _ffi.debug_path() == []                  # K = 0: nothing to launch
    with pytest.raises(ValueError):
        _ffi.lag_corr(np.ones(10), np.ones(8), 2)


# ---------------------------------------------------------------------------------------------------------------- sym_count_rows_dev
MODES = [(_ffi.SYM_QAM, M, k) for M in (2, 4, 8, 16) for k in range(4)] + [(_ffi.SYM_QPSK, 0, k) for k in range(4)] + [(_ffi.SYM_BPSK, 0, k) for k in range(2)]


def count_case(rng, mode, M, nrow, n, t0, r0, start, step, tdt, xdt):
    """rows a little wider than what is read; whatever a call does not read is loud"""
    wt, wx = t0 + n + 2, start + (r0 + n) * step + 3
    if mode == _ffi.SYM_QAM:
        sym = (2 * rng.integers(0, M, (nrow, n)) - (M - 1)) + 1j * (2 * rng.integers(0, M, (nrow, n)) - (M - 1))
        scale = M - 1
    else:
        sym = (2 * rng.integers(0, 2, (nrow, n)) - 1) + 1j * (2 * rng.integers(0, 2, (nrow, n)) - 1)
        scale = 1
    tx = loud(nrow * wt, np.complex128).reshape(nrow, wt)
    x = loud(nrow * wx, np.complex128, 17).reshape(nrow, wx)
    tx[:, t0:t0 + n] = sym
    x[:, start + (r0 + np.arange(n)) * step] = sym / scale + (0.9 / scale) * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))
    if np.dtype(tdt).kind != "c":
        tx = tx.real
    if np.dtype(xdt).kind != "c":
        x = x.real
    return tx.astype(tdt), x.astype(xdt)


def run_count(tx, x, mode, M, k, start, step, n, t0, r0):
    nrow = tx.shape[0]
    gt, gx, out = Guarded(tx, tx.dtype, 1 if tx.dtype != np.complex128 else 0), Guarded(x, x.dtype, 3 if x.dtype != np.complex128 else 0), GuardedOut(32 * nrow)
    try:
        _ffi.sym_count_rows_dev(gt.ptr, tx.dtype, tx.shape[1], t0, gx.ptr, x.dtype, x.shape[1], start, step, r0, n, nrow, mode, M, k, out.ptr)
        assert _ffi.debug_path() == (["symcount"] if n else [])
        return out.read(np.int64).reshape(nrow, 4)
    finally:
        for g in (gt, gx, out):
            g.free()


@pytest.mark.parametrize("nrow", (1, 3, 64))
def test_sym_count_rows_dev_equals_the_host_form(nrow):
    rng = np.random.default_rng(2520 + nrow)
    sizes = (1, 63, 64, 65, 4097)
    pairs = ((np.complex128, np.complex128), (np.complex64, np.complex64), (np.float64, np.complex64), (np.complex128, np.float32), (np.float32, np.float64))
    for i, (mode, M, k) in enumerate(MODES):
        for j, n in enumerate(sizes):
            if nrow == 64 and (i + j) % 3:
                continue                                              # (64 rows: a third of the grid, every mode and every size still met)
            tdt, xdt = pairs[(i + j) % len(pairs)]
            t0, r0, start, step = (1, 3, 0)[(i + j) % 3], (3, 0, 5)[j % 3], (0, 1)[i % 2], (1, 4)[(i + j) % 2]
            tx, x = count_case(rng, mode, M, nrow, n, t0, r0, start, step, tdt, xdt)
            want = _ffi.sym_count_rows_host(tx, x, mode, M, k, start, step, n, t0, r0)
            got = run_count(tx, x, mode, M, k, start, step, n, t0, r0)
            assert np.array_equal(got, want), (mode, M, k, n, nrow)
            assert not want[:, 3].any() and (n < 64 or want[:, 0].any())
    assert np.array_equal(run_count(tx, x, mode, M, k, start, step, 0, t0, r0), np.zeros((nrow, 4), dtype=np.int64))     # n = 0: zeros, no launch


def test_every_precondition_violation_is_counted_and_raises():
    rng = np.random.default_rng(2530)
    n = 2500
    for mode, M, spoil_tx in ((_ffi.SYM_QAM, 4, 0.5), (_ffi.SYM_QPSK, 0, 1e6), (_ffi.SYM_BPSK, 0, -7e4)):
        tx, x = count_case(rng, mode, M, 2, n, 0, 0, 0, 1, np.complex128, np.complex128)
        clean = run_count(tx, x, mode, M, 1, 0, 1, n, 0, 0)
        assert not clean[:, 3].any()
        rows_of = {_ffi.SYM_QAM: lambda t, r: dc.qam_sep_rows(t, r, '16qam', 1), _ffi.SYM_QPSK: lambda t, r: dc.qpsk_bep_rows(t, r, 1),
                   _ffi.SYM_BPSK: lambda t, r: dc.bpsk_bep_rows(t, r, 1)}[mode]
        assert np.array_equal(rows_of(tx[:, :n], x[:, :n])[1], clean[:, 0])
        for where, value in (("x", np.nan), ("x", np.inf), ("x", -np.inf), ("tx", spoil_tx), ("tx", np.nan)):
            t2, x2 = tx.copy(), x.copy()
            (x2 if where == "x" else t2)[1, 2049] = value
            want = _ffi.sym_count_rows_host(t2, x2, mode, M, 1, n=n)
            got = run_count(t2, x2, mode, M, 1, 0, 1, n, 0, 0)
            assert np.array_equal(got, want) and got[0, 3] == 0 and got[1, 3] == 1, (mode, where, value)
            with pytest.raises(ValueError, match="precondition"):
                rows_of(t2[:, :n], x2[:, :n])
    tx = (2 * rng.integers(0, 2, 2000) - 1) + 1j * (2 * rng.integers(0, 2, 2000) - 1)                # (a unique peak at lag 0: the overlap is everything)
    rx = tx.copy()
    for bad_rx in (np.nan, np.inf):
        r2 = rx.copy()
        r2[1500] = bad_rx
        with pytest.raises(ValueError):
            dc.qam_sep(tx, r2, 'qpsk')
        with pytest.raises(ValueError, match="finite|int16"):
            dc.qpsk_bep(tx, r2)
        with pytest.raises(ValueError, match="finite|int16"):
            dc.bpsk_bep(tx.real, r2.real)
    with pytest.raises(ValueError, match="integer"):
        dc.qam_sep(tx + 0.5, rx, 'qpsk')
    with pytest.raises(ValueError, match="zero energy"):
        dc.qam_sep(np.zeros(100), rx[:100], 'qpsk')
    with pytest.raises(ValueError, match="zero energy"):
        dc.xcorr(np.zeros(100), np.ones(100), 5)


# ---------------------------------------------------------------------------------------------------------------- the public functions
def sep_streams(c):
    t = G[c["key"] + "_tx"].astype(np.float64)
    return t[0] + 1j * t[1], G[c["key"] + "_rx"]


@pytest.mark.parametrize("c", XC, ids=[c["key"] for c in XC])
def test_xcorr_equals_the_fixture_and_the_host_form(c):
    x1, x2 = G[c["key"] + "_x1"], G[c["key"] + "_x2"]
    r, k = dc.xcorr(x1, x2, c["n_lags"])
    assert _ffi.debug_path() == ["lagcorr"]
    assert r.dtype == np.complex128 and k.dtype == np.int64 and np.array_equal(k, G[c["key"] + "_k"])
    print("xcorr", c["key"], float(np.max(np.abs(r - G[c["key"] + "_r"]))))
    assert np.max(np.abs(r - G[c["key"] + "_r"])) <= 1e-12 and np.max(np.abs(r - dc.xcorr_host(x1, x2, c["n_lags"])[0])) <= 1e-12
    d1, d2 = _ffi.DeviceArray.from_host(x1), _ffi.DeviceArray.from_host(x2)
    rd, kd = dc.xcorr(d1, d2, c["n_lags"])
    assert rd.tobytes() == r.tobytes() and np.array_equal(kd, k)
    d1.free()
    d2.free()


@pytest.mark.parametrize("c", SEP, ids=[c["key"] for c in SEP])
def test_qam_sep_equals_the_fixture_and_the_host_form(c, caplog):
    tx, rx = sep_streams(c)
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        got = dc.qam_sep(tx, rx, c["mod"], c["n_corr"], c["n_transient"])
    assert _ffi.debug_path() == ["lagcorr", "symcount"]
    lines = [r.getMessage() for r in caplog.records]
    assert lines == ['Phase ambiquity = (1j)**%d, taumax = %d' % (c["kmax"], c["taumax"]),
                     'Symbols = %d, Errors %d, SEP = %1.2e' % (c["nsymb"], c["nerr"], c["nerr"] / float(c["nsymb"]))]
    assert got == (c["nsymb"], c["nerr"], c["nerr"] / float(c["nsymb"])) == dc.qam_sep_host(tx, rx, c["mod"], c["n_corr"], c["n_transient"])
    assert [type(v) for v in got] == [int, int, float]
    for tdt, rdt in ((np.complex128, np.complex128), (np.complex64, np.complex128)):
        dt_, dr_ = _ffi.DeviceArray.from_host(tx.astype(tdt)), _ffi.DeviceArray.from_host(rx.astype(rdt))
        assert dc.qam_sep(dt_, dr_, c["mod"], c["n_corr"], c["n_transient"], SEP_disp=False) == got
        dt_.free()
        dr_.free()


@pytest.mark.parametrize("c", BPSK, ids=[c["key"] for c in BPSK])
def test_bpsk_bep_equals_the_fixture_and_the_host_form(c):
    tx, rx = G[c["key"] + "_tx"], G[c["key"] + "_rx"]
    got = dc.bpsk_bep(tx, rx, c["n_corr"], c["n_transient"])
    assert _ffi.debug_path() == ["symcount"]
    assert got == (c["count"], c["errors"]) == dc.bpsk_bep_host(tx, rx, c["n_corr"], c["n_transient"])
    assert type(got[0]) is int and isinstance(got[1], np.int64)
    d1, d2 = _ffi.DeviceArray.from_host(tx), _ffi.DeviceArray.from_host(rx)
    assert dc.bpsk_bep(d1, d2, c["n_corr"], c["n_transient"]) == got
    d1.free()
    d2.free()


@pytest.mark.parametrize("c", QPSK, ids=[c["key"] for c in QPSK])
def test_qpsk_bep_equals_the_host_form_at_the_injected_lag(c, caplog):
    tx, rx = G[c["key"] + "_tx"], G[c["key"] + "_rx"]
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        got = dc.qpsk_bep(tx, rx, c["n_corr"], c["n_transient"])
    assert [r.getMessage() for r in caplog.records] == ['kmax =  %d, taumax = %d' % (c["rot"], c["lag"])]
    assert got == dc.qpsk_bep_host(tx, rx, c["n_corr"], c["n_transient"]) and type(got[0]) is int and all(isinstance(v, np.int64) for v in got[1:])
    d1, d2 = _ffi.DeviceArray.from_host(tx), _ffi.DeviceArray.from_host(rx.astype(np.complex64))
    assert dc.qpsk_bep(d1, d2, c["n_corr"], c["n_transient"]) == dc.qpsk_bep_host(tx, rx.astype(np.complex64), c["n_corr"], c["n_transient"])
    d1.free()
    d2.free()


def test_rows_forms_equal_their_host_forms():
    rng = np.random.default_rng(2540)
    for mod, M in (('qpsk', 2), ('16qam', 4), ('64qam', 8), ('256qam', 16)):
        tx, x = count_case(rng, _ffi.SYM_QAM, M, 5, 2100, 0, 0, 3, 4, np.complex128, np.complex64)
        got, want = dc.qam_sep_rows(tx[:, :2100], x, mod, 2, 3, 4), dc.qam_sep_rows_host(tx[:, :2100], x, mod, 2, 3, 4)
        assert got[0] == want[0] == 2100 and np.array_equal(got[1], want[1]) and got[1].dtype == np.int64 and got[1].any()
    tx, x = count_case(rng, _ffi.SYM_QPSK, 0, 5, 2100, 0, 0, 0, 1, np.complex128, np.complex128)
    got, want = dc.qpsk_bep_rows(tx[:, :2100], x[:, :2100], 3), dc.qpsk_bep_rows_host(tx[:, :2100], x[:, :2100], 3)
    assert got[0] == want[0] == 2100 and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    got, want = dc.bpsk_bep_rows(tx[:, :2100].real, x[:, :2100].real, 1), dc.bpsk_bep_rows_host(tx[:, :2100].real, x[:, :2100].real, 1)
    assert got[0] == want[0] == 2100 and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="Unknown mod_type"):
        dc.qam_sep_rows(tx, x, '8psk')


# ---------------------------------------------------------------------------------------------------------------- a device-resident loop
def test_device_resident_16qam_loop_meets_its_host_form_and_theory():
    """16 rows x 65536 symbols of qam_bb's 16-QAM levels (+-1, +-3 per component, sent as +-1/3, +-1) -> awgn_rows_dev (seed 2550, sigma per
    component) -> the fused count, nothing on the host in between.  The counts equal the host form on the device's own draw
    (_ffi.awgn_rows_host).  Theory: a component is decided wrongly with probability p = 2 (1 - 1/4) Q(d / sigma), d = 1/3 half the level
    spacing, the symbol with 1 - (1 - p)^2; sigma = d / 2.17, i.e. Es/N0 = (10/9) / (2 sigma^2) = 13.7 dB.  The total of 2^20 symbols must lie
    within 4 binomial standard deviations."""
    nrow, n, seed = 16, 65536, 2550
    rng = np.random.default_rng(seed)
    tx = ((2 * rng.integers(0, 4, (nrow, n)) - 3) + 1j * (2 * rng.integers(0, 4, (nrow, n)) - 3)).astype(np.complex128)
    sigma = (1.0 / 3) / 2.17
    txd, xd, cnt = _ffi.DeviceArray.from_host(tx.reshape(-1)), _ffi.DeviceArray.from_host((tx / 3).reshape(-1)), _ffi.DeviceBytes(32 * nrow)
    _ffi.debug_path()
    _ffi.awgn_rows_dev(xd, xd, n, nrow, seed, sigma=sigma)
    _ffi.sym_count_rows_dev(txd, tx.dtype, n, 0, xd, tx.dtype, n, 0, 1, 0, n, nrow, _ffi.SYM_QAM, 4, 0, cnt)
    assert _ffi.debug_path() == ["awgn", "symcount"]
    got = cnt.read().view(np.int64).reshape(nrow, 4)
    noisy = _ffi.awgn_rows_host(tx / 3, 1.0, sigma, seed, np.complex128)
    assert np.array_equal(got, _ffi.sym_count_rows_host(tx, noisy, _ffi.SYM_QAM, 4, 0))
    assert np.array_equal(dc.qam_sep_rows(tx, noisy, '16qam')[1], got[:, 0]) and not got[:, 1:].any()
    p = 2 * (1 - 1 / 4) * 0.5 * math.erfc(2.17 / math.sqrt(2))
    ser = 1 - (1 - p) ** 2
    total, N = int(got[:, 0].sum()), nrow * n
    print("16-QAM loop: %d errors in %d symbols, theory %.1f +- %.1f" % (total, N, N * ser, math.sqrt(N * ser * (1 - ser))))
    assert abs(total - N * ser) <= 4 * math.sqrt(N * ser * (1 - ser))
    for d in (txd, xd, cnt):
        d.free()
