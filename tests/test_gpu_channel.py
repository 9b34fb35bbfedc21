"""The AWGN channel and the bit sources on the device (csrc/channel.hip): every _dev entry against its NumPy restatement bit for bit
(lengths around every chunk and work-item edge, 1 and 3 rows, strides, element-aligned windows off a 16-byte boundary, far stream indices,
all dtypes, in place, split calls, repeated runs), the rows' sigma and gain against the host formula, the public functions against every
g23 case, the footprint of every entry inside loud and NaN pads, the device-resident BER loop against its host restatement and against
theory, and an m-sequence source against itself one period on.  Bounds: DESIGN.md 4.18."""
import numpy as np
import pytest

from _pads import loud
from sk_dsp_comm_amd import _ffi, digitalcom as dc, sigsys as ss
import _channel as ch

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 4099)
FIRSTS = (0, 5, 2 ** 40 + 3)
PAIRS = ((np.float32, np.float32), (np.float64, np.float64), (np.complex64, np.complex64), (np.complex128, np.complex128),
         (np.float32, np.complex64), (np.float64, np.complex128))
PAD = 4096      # bytes in front of and behind every window: a multiple of 256, more than a work item's chunk run can overshoot by a vector
FILL = 0xEE


@pytest.fixture(scope="module", autouse=True)
def _device():
    _ffi.init(0)


def signal(rng, shape, dt):
    x = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dt)


class Window:
    """rows of `dt`, `stride` elements apart, `off` elements behind a 256-byte boundary, inside pads of PAD bytes on the device"""

    def __init__(self, dt, n, nrow, stride, off, rows=None, pad=None):
        self.dt, self.n, self.nrow, self.stride, self.off = np.dtype(dt), n, nrow, stride, off
        esz = self.dt.itemsize
        span = (nrow - 1) * stride + n
        host = np.full(2 * PAD + (off + span) * esz + 64, FILL, dtype=np.uint8)
        if pad is not None:
            body = host[:host.size // esz * esz].view(self.dt)
            body[:] = pad(body.size, self.dt)
        self.first = PAD + off * esz
        self.own = np.zeros(host.size, dtype=bool)
        for r in range(nrow):
            lo = self.first + r * stride * esz
            self.own[lo:lo + n * esz] = True
            if rows is not None:
                host[lo:lo + n * esz] = np.ascontiguousarray(rows[r], dtype=self.dt).view(np.uint8)
        self.before = host.copy()
        self.dev = _ffi.device_bytes_of(host)
        self.ptr = self.dev.ptr + self.first

    def rows(self, untouched_outside=True):
        raw = self.dev.read()
        if untouched_outside:
            assert np.array_equal(raw[~self.own], self.before[~self.own]), "bytes outside the rows changed"
        esz = self.dt.itemsize
        return np.stack([raw[self.first + r * self.stride * esz:self.first + (r * self.stride + self.n) * esz].view(self.dt) for r in range(self.nrow)])

    def free(self):
        self.dev.free()


def dev_awgn(x, ydt, g, sigma, seed, first=0, frow=0, xo=0, yo=0, inplace=False, per_row=True, pad=None):
    nrow, n = x.shape
    xw = Window(x.dtype, n, nrow, n + 1, xo, x, pad)
    yw = xw if inplace else Window(ydt, n, nrow, n + 3, yo)
    gd = sd = None
    if per_row:
        gd, sd = _ffi.DeviceArray.from_host(np.asarray(g, dtype=np.float64)), _ffi.DeviceArray.from_host(np.asarray(sigma, dtype=np.float64))
    _ffi.awgn_rows_dev(xw.ptr, yw.ptr, n, nrow, seed, g=float(np.ravel(g)[0]), sigma=float(np.ravel(sigma)[0]), gd=gd, sd=sd, x_stride=xw.stride, y_stride=yw.stride,
                       first_index=first, first_row=frow, x_dtype=x.dtype, y_dtype=ydt)
    y = yw.rows()
    if not inplace:
        assert np.array_equal(xw.dev.read(), xw.before), "the input changed"
        yw.free()
    xw.free()
    return y


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- device = host, bit for bit
@pytest.mark.parametrize("xdt,ydt", PAIRS)
def test_awgn_rows_dev_equals_the_host_form(xdt, ydt):
    rng = np.random.default_rng(2310)
    for li, n in enumerate(LENGTHS):
        for nrow in (1, 3):
            x = signal(rng, (nrow, n), xdt)
            g, sigma = rng.uniform(0.5, 2.0, nrow), rng.uniform(0.1, 3.0, nrow)
            first, frow = FIRSTS[(li + nrow) % 3], (0, 2 ** 31)[li % 2]
            xo, yo = (li + 1) % max(1, 16 // np.dtype(xdt).itemsize), (li + nrow) % max(1, 16 // np.dtype(ydt).itemsize)
            per_row = bool((li + nrow) % 2) or nrow > 1
            want = _ffi.awgn_rows_host(x, g, sigma, 77, ydt, first, frow)
            assert same_bits(dev_awgn(x, ydt, g, sigma, 77, first, frow, xo, yo, per_row=per_row), want), (n, nrow, first, "sqrt, ln or sincos differ on the device?")
            if xdt == ydt:
                assert same_bits(dev_awgn(x, ydt, g, sigma, 77, first, frow, yo, yo, inplace=True, per_row=per_row), want), ("in place", n, nrow)


def dev_bits(kind, n, nrow, yo, seed=0, first=0, frow=0, x=None, sigma=None, xo=0, inplace=False, period=None, phases=None, pad=None):
    yw = Window(np.uint8, n, nrow, n + 5, yo, x if inplace else None)
    extra = []
    if kind == "rbits":
        _ffi.random_bits_rows_dev(yw.ptr, n, nrow, seed, y_stride=yw.stride, first_index=first, first_row=frow)
    elif kind == "abits":
        xw = yw if inplace else Window(np.uint8, n, nrow, n + 1, xo, x, pad)
        sd = _ffi.DeviceArray.from_host(np.asarray(sigma, dtype=np.float64))
        _ffi.awgn_bits_rows_dev(xw.ptr, yw.ptr, n, nrow, seed, sd=sd, x_stride=xw.stride, y_stride=yw.stride, first_index=first, first_row=frow)
        extra = [sd] + ([] if inplace else [xw])
        if not inplace:
            assert np.array_equal(xw.dev.read(), xw.before)
    else:
        cd, pd = _ffi.device_bytes_of(period), _ffi.device_bytes_of(np.asarray(phases, dtype=np.int64))
        _ffi.pn_rows_dev(cd, period.size, yw.ptr, n, nrow, phases_d=pd, y_stride=yw.stride, first_index=first)
        extra = [cd, pd]
    y = yw.rows()
    for d in extra + [yw]:
        d.free()
    return y


def test_bit_kernels_equal_the_host_forms():
    rng = np.random.default_rng(2311)
    c5, c16 = ss._mseq_bytes(5), ss._mseq_bytes(16)
    for li, n in enumerate(LENGTHS):
        for nrow in (1, 3):
            yo, first, frow = (5 * li + nrow) % 16, (FIRSTS + (121,))[(li + nrow) % 4], (0, 2 ** 31)[li % 2]
            want = np.stack([_ffi.random_bits_host(99, frow + r, first, n) for r in range(nrow)])
            assert np.array_equal(dev_bits("rbits", n, nrow, yo, 99, first, frow), want), ("rbits", n, nrow)
            x, sigma = rng.integers(0, 2, (nrow, n)).astype(np.uint8), rng.uniform(0.3, 1.5, nrow)
            want = _ffi.awgn_bits_rows_host(x, sigma, 98, first, frow)
            assert np.array_equal(dev_bits("abits", n, nrow, yo, 98, first, frow, x, sigma, xo=(yo + 3 * li) % 16), want), ("abits", n, nrow)
            assert np.array_equal(dev_bits("abits", n, nrow, yo, 98, first, frow, x, sigma, inplace=True), want), ("abits in place", n, nrow)
            for c in (c5, c16):
                phases = [(0, c.size - 1, c.size // 2)[(r + li) % 3] for r in range(nrow)]
                want = np.stack([c[(ph + first + np.arange(n, dtype=np.int64)) % c.size] for ph in phases])
                assert np.array_equal(dev_bits("pn", n, nrow, yo, first=first, period=c, phases=phases), want), ("pn", c.size, n, nrow)


def test_two_calls_over_a_split_equal_one_call_and_runs_repeat():
    rng = np.random.default_rng(2312)
    n, n1, nrow = 4099, 1237, 3
    for xdt, ydt in PAIRS[1:4]:
        x = signal(rng, (nrow, n), xdt)
        g, sigma = rng.uniform(0.5, 2.0, nrow), rng.uniform(0.1, 3.0, nrow)
        whole = dev_awgn(x, ydt, g, sigma, 5, 5, 1)
        assert same_bits(whole, dev_awgn(x, ydt, g, sigma, 5, 5, 1))
        parts = [dev_awgn(np.ascontiguousarray(x[:, :n1]), ydt, g, sigma, 5, 5, 1), dev_awgn(np.ascontiguousarray(x[:, n1:]), ydt, g, sigma, 5, 5 + n1, 1)]
        assert same_bits(whole, np.concatenate(parts, axis=1))
        rows = [dev_awgn(x[r:r + 1], ydt, g[r:r + 1], sigma[r:r + 1], 5, 5, 1 + r) for r in range(nrow)]      # first_row: a window of the rows
        assert same_bits(whole, np.concatenate(rows, axis=0))
    whole = dev_bits("rbits", n, nrow, 3, 6, 121, 2)
    assert np.array_equal(whole, dev_bits("rbits", n, nrow, 9, 6, 121, 2))
    assert np.array_equal(whole, np.concatenate([dev_bits("rbits", n1, nrow, 1, 6, 121, 2), dev_bits("rbits", n - n1, nrow, 2, 6, 121 + n1, 2)], axis=1))
    x = rng.integers(0, 2, (nrow, n)).astype(np.uint8)
    whole = dev_bits("abits", n, nrow, 3, 6, 7, 0, x, [0.5, 0.7, 0.9])
    parts = [dev_bits("abits", n1, nrow, 1, 6, 7, 0, np.ascontiguousarray(x[:, :n1]), [0.5, 0.7, 0.9]),
             dev_bits("abits", n - n1, nrow, 2, 6, 7 + n1, 0, np.ascontiguousarray(x[:, n1:]), [0.5, 0.7, 0.9])]
    assert np.array_equal(whole, np.concatenate(parts, axis=1))


# ---------------------------------------------------------------------------------------------------------------- sigma and gain
@pytest.mark.parametrize("dt", (np.float32, np.float64, np.complex64, np.complex128))
def test_sigma_and_gain_per_row_against_the_host_formula(dt):
    """within 1e-13 relative: the documented bound of the merge of partial moments, a DC-offset row included"""
    rng = np.random.default_rng(2313)
    for n in (2, 17, 2049, 70001):
        x = signal(rng, (4, n), dt)
        x[1] += 10.0 * np.std(x[1])                                  # a DC offset of ten standard deviations
        x[2] *= 1e-3
        x[3] = 2.5 - (1.25j if np.dtype(dt).kind == "c" else 0)       # a constant row (every partial sum exact): variance 0
        var = np.var(x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64), axis=1)
        xw = Window(dt, n, 4, n + 1, 1 if np.dtype(dt).itemsize < 16 else 0, x, loud)
        for mode, ns, es, vw in ((_ffi.SIGMA_AWGN, 1, 10, 0.0), (_ffi.SIGMA_AWGN, 8, 0, 0.0), (_ffi.SIGMA_AWGN2, 8, 40, -40.0), (_ffi.SIGMA_AWGN2, 1, 10, 0.0)):
            gd, sd = _ffi.DeviceArray(4, np.float64), _ffi.DeviceArray(4, np.float64)
            _ffi.awgn_sigma_rows_dev(xw.ptr, n, 4, mode, ns, es, gd, sd, var_w_dB=vw, x_stride=xw.stride, dtype=dt)
            g, s = gd.to_host(), sd.to_host()
            wg, ws = _ffi.awgn_sigma_host(var, mode, ns, es, vw)
            assert var[3] == 0.0 and (s[3] == 0.0 if mode == _ffi.SIGMA_AWGN else np.isinf(g[3]))
            assert np.all(np.abs(g[:3] - wg[:3]) <= 1e-13 * np.abs(wg[:3])) and np.all(np.abs(s[:3] - ws[:3]) <= 1e-13 * np.abs(ws[:3])), (n, mode, g, wg, s, ws)
            if mode == _ffi.SIGMA_AWGN:
                assert np.all(g == 1.0)
            else:
                assert np.all(s == ws)                              # sqrt(var_w / 2): no variance in it
            gd.free(), sd.free()
        assert np.array_equal(xw.dev.read(), xw.before)
        xw.free()
    xn = np.array([[1.0, np.nan, 2.0]], dtype=dt)
    gd, sd, xd = _ffi.DeviceArray(1, np.float64), _ffi.DeviceArray(1, np.float64), _ffi.DeviceArray.from_host(xn.reshape(-1))
    _ffi.awgn_sigma_rows_dev(xd, 3, 1, _ffi.SIGMA_AWGN, 1, 10, gd, sd)
    assert np.isnan(sd.to_host()[0])                                 # NaN propagates, as np.var's does


# ---------------------------------------------------------------------------------------------------------------- the public functions
def test_public_functions_against_every_g23_case():
    g, lists = ch.g23()
    for case in lists["awgn"]:
        ch.check_awgn_case(g, case, ss.cpx_awgn if case["fn"] == "cpx_awgn" else ss.cpx_awgn2)
    for case in lists["chan"]:
        ch.check_chan_case(g, case, dc.awgn_channel)
    for p in lists["pn"]:
        y = ss.pn_gen(p["n_bits"], p["m"])
        assert y.dtype == np.float64 and np.array_equal(y, np.unpackbits(g[p["key"]])[:p["n_bits"]])
    _ffi.debug_path()
    assert np.array_equal(ss.pn_gen(70000, 16), ss.pn_gen_host(70000, 16)) and "pn" in _ffi.debug_path()       # past 2^16: from the kernel
    x = signal(np.random.default_rng(2314), (3, 1000), np.complex128)
    x[1] *= 7.0
    rows = ss.cpx_awgn_rows(x, 10, 8, seed=11)
    var = np.var(x, axis=1)
    want = _ffi.awgn_rows_host(x, *_ffi.awgn_sigma_host(var, _ffi.SIGMA_AWGN, 8, 10), 11)
    assert rows.dtype == np.complex128 and np.max(np.abs(rows - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(ss.cpx_awgn(x[0], 10, 8, seed=11) - want[0])) <= 1e-12 * np.max(np.abs(want))               # row 0 of the rows form is the 1-D call
    bits = ss.random_bits_rows(3, 1000, seed=12)
    assert bits.dtype == np.uint8 and np.array_equal(bits, np.stack([_ffi.random_bits_host(12, r, 0, 1000) for r in range(3)]))
    assert np.array_equal(dc.awgn_channel_rows(bits, 2.0, seed=13), _ffi.awgn_bits_rows_host(bits, dc._channel_sigma(2.0), 13))
    c = ss._mseq_bytes(7)
    assert np.array_equal(ss.pn_rows(2, 300, 7, phases=[0, 126]), np.stack([c[(ph + np.arange(300)) % 127] for ph in (0, 126)]))
    np.random.seed(5)
    a = ss.cpx_awgn(np.arange(16.0), 3, 1)
    np.random.seed(5)
    assert np.array_equal(a, ss.cpx_awgn(np.arange(16.0), 3, 1)) and not np.array_equal(a, ss.cpx_awgn(np.arange(16.0), 3, 1))


# ---------------------------------------------------------------------------------------------------------------- footprint
def nan_pad(count, dt):
    return np.full(count, np.nan, dtype=dt)


def test_every_entry_reads_only_its_window_and_writes_only_its_rows():
    """inputs inside loud and NaN pads (tests/_pads.py), the row gaps included: the same bytes come out, and Window.rows finds every byte
    around the output rows as it was"""
    rng = np.random.default_rng(2315)
    n, nrow = 2049, 3
    for xdt, ydt in PAIRS:
        x = signal(rng, (nrow, n), xdt)
        outs = [dev_awgn(x, ydt, [1.0, 0.5, 2.0], [0.3, 0.6, 0.9], 21, 5, 0, xo=1 if np.dtype(xdt).itemsize < 16 else 0, yo=1 if np.dtype(ydt).itemsize < 16 else 0, pad=pad)
                for pad in (None, lambda c, dt: loud(c, dt), nan_pad)]
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]) and np.all(np.isfinite(outs[0])), (xdt, ydt)
    x = rng.integers(0, 2, (nrow, n)).astype(np.uint8)
    outs = [dev_bits("abits", n, nrow, 7, 22, 5, 0, x, [0.5, 0.7, 0.9], xo=3, pad=pad) for pad in (None, lambda c, dt: np.full(c, 0xA5, dtype=dt))]
    assert np.array_equal(outs[0], outs[1]) and outs[0].max() <= 1


# ---------------------------------------------------------------------------------------------------------------- the loop, device-resident
@pytest.mark.parametrize("mod,es_n0", ch.LOOP_CASES)
def test_ber_loop_stays_on_the_device_and_meets_theory(mod, es_n0):
    """16 rows x 65536 symbols: random bits -> MPSK Gray map -> sigma and gain of every row -> channel (in place) -> demap -> count, nothing
    but the 16 counts crossing to the host.  The counts equal the host restatement of the same loop exactly, and the total lies within
    5 sqrt(n p (1 - p)) of n p, p = 1/2 erfc(sqrt(Eb/N0)).  Order 2: 13046 of 1048576 (expected 13108.1); order 4: 26359 of 2097152 (26396.9)."""
    nrow, nsym, bps = ch.LOOP_ROWS, ch.LOOP_SYMS, _ffi.sym_bits(_ffi.MPSK, mod)
    nb = bps * nsym
    bits, rx, cnt = _ffi.DeviceBytes(nrow * nb), _ffi.DeviceBytes(nrow * nb), _ffi.DeviceBytes(8 * nrow)
    sym, gd, sd = _ffi.DeviceArray(nrow * nsym, np.complex128), _ffi.DeviceArray(nrow, np.float64), _ffi.DeviceArray(nrow, np.float64)
    _ffi.random_bits_rows_dev(bits, nb, nrow, ch.LOOP_SEED)
    _ffi.gray_map_rows_dev(bits.ptr, nb, nsym, nrow, _ffi.MPSK, mod, np.complex128, sym.ptr)
    _ffi.awgn_sigma_rows_dev(sym, nsym, nrow, _ffi.SIGMA_AWGN, 1, es_n0, gd, sd)
    _ffi.awgn_rows_dev(sym, sym, nsym, nrow, ch.LOOP_SEED + 1, gd=gd, sd=sd)
    _ffi.gray_demap_rows_dev(sym.ptr, nsym, 0, 1, nsym, nrow, np.complex128, _ffi.MPSK, mod, rx.ptr)
    _ffi.bit_count_rows_dev(bits.ptr, nb, rx.ptr, nb, nb, nrow, ch.loop_inverts(mod), cnt.ptr)
    counts = cnt.read().view(np.int64)
    for d in (bits, rx, cnt, sym, gd, sd):
        d.free()
    n, p = ch.loop_expected(mod, es_n0)
    print("order %d: %d errors of %d bits, expected %.1f +- %.1f" % (mod, counts.sum(), n, n * p, np.sqrt(n * p * (1 - p))))
    assert np.array_equal(counts, ch.loop_host(mod, es_n0))
    assert ch.within_five_sigma(int(counts.sum()), n, p)


def test_pn_source_against_itself_one_period_on():
    """two rows of the same m-sequence, the second read one period further on: bit_errors_rows finds no difference"""
    for m in (5, 16):
        c = ss._mseq_bytes(m)
        q, n = c.size, 3 * c.size + 11
        cd, a, b = _ffi.device_bytes_of(c), _ffi.DeviceBytes(n), _ffi.DeviceBytes(n)
        _ffi.pn_rows_dev(cd, q, a, n, 1, first_index=0)
        _ffi.pn_rows_dev(cd, q, b, n, 1, first_index=q)
        tx, rx = a.read()[None, :], b.read()[None, :]
        count, errors = dc.bit_errors_rows(tx, rx)
        assert count == n and errors.tolist() == [0] and np.array_equal(tx[0], np.resize(c, n))
        count, errors = dc.bit_errors_rows(tx[:, :-1], rx[:, 1:])       # one bit on instead: the count does see a shift
        assert count == n - 1 and errors[0] > n // 4
        for d in (cd, a, b):
            d.free()
