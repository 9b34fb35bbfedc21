"""OFDM on the GPU (csrc/ofdm.hip): the _dev entry points against the float64 _host restatements over a sparse product of sizes, prefixes, pilot
periods, symbol counts, rows, alignments and dtypes, every call inside loud or NaN pads whose bytes must come back unchanged; repeatability,
NaN containment, chan_est_equalize, the public functions against every result captured from the real reference (g24_ofdm.npz), and the
device-resident loop bits -> 16-QAM -> OFDM tx -> AWGN -> OFDM rx -> demap -> count.  Tolerances: DESIGN.md 4.19 (tests/_ofdm.py)."""
import numpy as np
import pytest
from scipy import signal

from sk_dsp_comm_amd import _ffi, digitalcom as dc
import _ofdm as of
from _pads import loud

pytestmark = pytest.mark.gpu

PAD = 38                                       # elements in front of and behind the rows (even: `off` alone decides the 16-byte alignment)
NCS = (64, 128, 256, 512, 1024, 2048, 4096)


def nan_pad(count, dt):
    return np.full(count, np.nan + 1j * np.nan, dtype=dt)


class Rows:
    """nrow rows of n elements, n + 1 apart, `off` elements behind a pad, inside one device allocation whose other elements hold pad values"""

    def __init__(self, nrow, n, dt, off, pad, x2d=None):
        self.nrow, self.n, self.dt, self.stride, self.start = nrow, n, np.dtype(dt), n + 1, PAD + off
        total = self.start + (nrow - 1) * self.stride + n + PAD
        self.img = pad(total, dt)
        self.own = np.zeros(total, dtype=bool)
        for r in range(nrow):
            lo = self.start + r * self.stride
            self.own[lo:lo + n] = True
            if x2d is not None:
                self.img[lo:lo + n] = x2d[r]
        self.dev = _ffi.DeviceArray.from_host(self.img)
        self.ptr = self.dev.ptr + self.start * self.dt.itemsize

    def rows(self):
        """the rows after a call; every other byte of the allocation must be what it was"""
        now = self.dev.to_host()
        assert np.array_equal(now[~self.own].view(np.uint8), self.img[~self.own].view(np.uint8)), "a byte outside the rows changed"
        return np.stack([now[self.start + r * self.stride:self.start + r * self.stride + self.n] for r in range(self.nrow)])

    def free(self):
        self.dev.free()


def dev_tx(data, nf, nc, npb, cp, ncp, off=0, pad=loud):
    nrow, nsym = data.shape[0], data.shape[1] // nf
    x = Rows(nrow, nsym * nf, data.dtype, off, pad, data)
    y = Rows(nrow, _ffi.ofdm_tx_symbols(nsym, npb) * (nc + (ncp if cp else 0)), data.dtype, 1 - off if data.dtype == np.complex64 else 0, pad)
    _ffi.ofdm_tx_rows_dev(x.ptr, y.ptr, nsym, nrow, nf, nc, npb, cp, ncp, x.stride, y.stride, data.dtype)
    out = y.rows()
    x.rows()
    x.free(), y.free()
    return out


def dev_rx(rx, nsym, nf, nc, npb, cp, ncp, alpha, hht, off=0, pad=loud):
    nrow = rx.shape[0]
    x = Rows(nrow, rx.shape[1], rx.dtype, off, pad, rx)
    z = Rows(nrow, _ffi.ofdm_rx_data_symbols(nsym, npb) * nf, rx.dtype, 1 - off if rx.dtype == np.complex64 else 0, pad)
    h = Rows(1, nrow * nf, np.complex128, 0, pad)
    _ffi.ofdm_rx_rows_dev(x.ptr, z.ptr, nsym, nrow, nf, nc, npb, cp, ncp, alpha, hht, h.ptr if npb > 0 else None, x.stride, z.stride, rx.dtype)
    out, hh = z.rows(), h.rows().reshape(nrow, nf)
    x.rows()
    x.free(), z.free(), h.free()
    return out, hh


def hht_of(nf, nc):
    Ht = np.fft.fft(of.HC, nc)
    return np.hstack((Ht[1:nf // 2 + 1], Ht[nc - nf // 2:]))


def sparse_cases():
    """(nc, nf, symbols, npb, cp, ncp, nrow, dtype, off): every value of every axis of the issue's grid, each nc with every symbol count"""
    out = []
    for i, nc in enumerate(NCS):
        nb = max(1, 1024 // nc)
        for j, nsym in enumerate(sorted({1, nb - 1, nb, nb + 1, 2 * nb + 1} - {0})):
            k = i + j
            out.append((nc, (2, nc // 2, nc - 2)[k % 3], nsym, (0, 2, 3, 10)[(i + 2 * j) % 4]) + ((True, 0), (True, 1), (True, 10), (True, nc), (False, 7))[(2 * i + j) % 5] +
                       ((1, 3)[k % 2], (np.complex128, np.complex64)[(k // 2) % 2], (k // 3) % 2))
    return out


def run_case(case, pad=loud):
    """transmitter, then all four receiver modes on its output through the channel; returns everything the device produced"""
    nc, nf, nsym, npb, cp, ncp, nrow, dt, off = case
    rng = np.random.default_rng(hash((nc, nf, nsym, npb, ncp)) % 2 ** 31)
    data = of.qam16(rng, (nrow, nsym * nf)).astype(dt)
    want = np.stack([dc.ofdm_tx_host(r, nf, nc, npb, cp, ncp) for r in data])
    got = [dev_tx(data, nf, nc, npb, cp, ncp, off, pad)]
    errs = [of.close(got[0], want.astype(np.complex128), ("tx",) + case[:6])]
    full = np.stack([signal.lfilter(of.HC, 1, r) for r in want.astype(np.complex128)]).astype(dt)
    rsym = full.shape[1] // (nc + ncp)
    if rsym:
        used = np.ascontiguousarray(full[:, :rsym * (nc + ncp if cp else nc)])
        for rnpb, ht in ((0, None), (-1, of.HC), (npb if npb else 3, of.HC), (npb if npb else 2, None)):
            ref = [dc.ofdm_rx_host(r.astype(np.complex128), nf, nc, rnpb, cp, ncp, 0.9, ht) for r in full]
            z, h = dev_rx(used, rsym, nf, nc, rnpb, cp, ncp, 0.9, None if ht is None else hht_of(nf, nc), off, pad)
            errs.append(of.close(z, np.stack([r[0] for r in ref]), ("rx", rnpb, ht is None) + case[:6], 1 / 0.45))
            assert np.all(np.isfinite(z))
            if rnpb > 0:
                of.close(h, np.stack([r[1] for r in ref]), ("H", rnpb) + case[:6])
                got.append(h)
            got.append(z)
    assert np.all(np.isfinite(got[0]))
    return got, max(errs)


@pytest.mark.parametrize("nc", NCS)
def test_dev_entries_equal_the_host_forms(nc):
    worst = 0.0
    for case in [c for c in sparse_cases() if c[0] == nc]:
        _ffi.debug_path()
        worst = max(worst, run_case(case)[1])
        assert "ofdm_tx" in _ffi.debug_path()
    print("nc = %d: worst relative error %.2e" % (nc, worst))


def test_footprint_inside_loud_and_nan_pads_and_repeatability():
    """the same cases inside loud pads, inside NaN pads and once more: identical bytes every time (Rows.rows finds every byte around the rows as
    it was, and run_case that every output is finite: no pad value reaches one)"""
    for case in [c for c in sparse_cases() if c[0] in (64, 512, 2048)][::2]:
        a, b, c = run_case(case, loud)[0], run_case(case, nan_pad)[0], run_case(case, loud)[0]
        for u, v, w in zip(a, b, c):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)) and np.array_equal(u.view(np.uint8), w.view(np.uint8)), case


def test_a_nan_stays_in_its_own_symbol():
    """npb = 0: a NaN in one input symbol makes exactly that symbol's outputs non-finite and no other (the reference's behaviour)"""
    rng = np.random.default_rng(2402)
    for nc, nf, nsym, ncp, bad in ((64, 32, 35, 8, 17), (512, 510, 5, 0, 1), (4096, 2, 3, 3, 2)):
        for dt in (np.complex128, np.complex64):
            data = of.qam16(rng, (2, nsym * nf)).astype(dt)
            data[1, bad * nf + nf - 1] = np.nan
            y = dev_tx(data, nf, nc, 0, True, ncp).reshape(2, nsym, nc + ncp)
            fin = np.isfinite(y)
            assert fin[0].all() and not fin[1, bad].any() and fin[1, np.arange(nsym) != bad].all(), (nc, dt)
            x = of.qam16(rng, (2, nsym * (nc + ncp))).astype(dt)
            x[0, bad * (nc + ncp) + ncp + 5] = np.nan
            z = dev_rx(x, nsym, nf, nc, 0, True, ncp, 0.9, None)[0].reshape(2, nsym, nf)
            fin = np.isfinite(z)
            assert fin[1].all() and not fin[0, bad].any() and fin[0, np.arange(nsym) != bad].all(), (nc, dt)


def test_chan_est_equalize_equals_its_host_form():
    rng = np.random.default_rng(2403)
    for dt in (np.complex128, np.complex64):
        for nsym, nf, npb, use_ht in ((11, 6, 3, False), (10, 300, 10, True), (7, 32, 2, False), (9, 2, 4, True), (1, 8, 5, False), (41, 4094, 10, False)):
            z = (rng.standard_normal((nsym, nf)) + 1j * rng.standard_normal((nsym, nf)) + 2).astype(dt)
            if npb == 10:
                z[-1] = 0                      # the trailing zero row of the multiplex: a "pilot" that scales H by alpha
            ht = rng.standard_normal(nf) + 1j * rng.standard_normal(nf) + 3 if use_ht else None
            zz, H = dc.chan_est_equalize(z, npb, 0.9, ht)
            rz, rH = dc.chan_est_equalize_host(z.astype(np.complex128), npb, 0.9, ht)
            assert zz.dtype == dt and H.dtype == np.complex128 and H.shape == (nf,)
            of.close(zz, rz, ("zz", nsym, nf, npb))
            of.close(H, rH, ("H", nsym, nf, npb))
    # the _dev entry on three rows of a wider buffer
    nsym, nf, npb, nrow = 9, 30, 4, 3
    z = (rng.standard_normal((nrow, nsym * nf)) + 1j * rng.standard_normal((nrow, nsym * nf)) + 2).astype(np.complex64)
    x, o, h = Rows(nrow, nsym * nf, np.complex64, 1, loud, z), Rows(nrow, _ffi.ofdm_rx_data_symbols(nsym, npb) * nf, np.complex64, 0, loud), Rows(1, nrow * nf, np.complex128, 0, loud)
    _ffi.ofdm_equalize_rows_dev(x.ptr, o.ptr, nsym, nrow, nf, npb, 0.9, h.ptr, None, x.stride, o.stride, np.complex64)
    ref = [dc.chan_est_equalize_host(r.reshape(nsym, nf).astype(np.complex128), npb, 0.9) for r in z]
    of.close(o.rows(), np.stack([r[0].reshape(-1) for r in ref]), "rows zz")
    of.close(h.rows().reshape(nrow, nf), np.stack([r[1] for r in ref]), "rows H")
    x.rows()
    x.free(), o.free(), h.free()


def test_public_functions_equal_the_reference():
    g, _, cases = of.g24()
    for case in cases:
        _ffi.debug_path()
        e = max(of.check_case_tx(g, case, dc.ofdm_tx), of.check_case_rx(g, case, dc.ofdm_rx))
        path = _ffi.debug_path()
        assert ("ofdm_tx" in path and "ofdm_rx" in path) == (case["nc"] != 96 and case["symbols"] > 0), (case["key"], path)
        print("%s: %.2e" % (case["key"], e))
    case = cases[0]
    data = g[case["key"] + "_data"]
    y = dc.ofdm_tx(data.astype(np.complex64), case["nf"], case["nc"], case["npb"], case["cp"], case["ncp"])
    assert y.dtype == np.complex64
    of.close(y, g[case["key"] + "_tx"], "complex64 tx")
    # a frame set: each row equals the 1-D call
    rows = np.stack([data[:3200], data[3:3203]])
    y2 = dc.ofdm_tx_rows(rows, 32, 64, 10, True, 8)
    assert np.array_equal(y2[1], dc.ofdm_tx(rows[1], 32, 64, 10, True, 8))
    z2, H2 = dc.ofdm_rx_rows(y2, 32, 64, 10, True, 8, alpha=0.9)
    z1, H1 = dc.ofdm_rx(y2[1], 32, 64, 10, True, 8, alpha=0.9)
    assert np.array_equal(z2[1], z1) and np.array_equal(H2[1], H1) and H2.shape == (2, 32)
    of.close(z2, rows, "tx -> rx with the estimator", 1 / 0.45)


def test_device_resident_loop():
    """4 rows x 64 symbols of nc = 64, nf = 32, ncp = 8: random bits -> 16-QAM Gray map -> OFDM tx -> AWGN (in place) -> OFDM rx -> scale ->
    demap -> count, nothing but the counts crossing to the host.  Without noise the count is exactly 0; with noise the per-row counts equal the
    host restatement's on the same draw, whose decision variables stay 1e-9 clear of every threshold (asserted first, on the host alone)."""
    want, margin = of.loop_host(of.LOOP_SIGMA)
    assert margin >= 1e-9 and want.sum() > 0
    nrow, nq = of.LOOP_ROWS, of.LOOP_SYMS * of.LOOP_NF
    nb, nt = 4 * nq, of.LOOP_SYMS * (of.LOOP_NC + of.LOOP_NCP)
    bits, rx, cnt = _ffi.DeviceBytes(nrow * nb), _ffi.DeviceBytes(nrow * nb), _ffi.DeviceBytes(8 * nrow)
    sym, tx, z, r = (_ffi.DeviceArray(nrow * nq, np.complex128), _ffi.DeviceArray(nrow * nt, np.complex128), _ffi.DeviceArray(nrow * nq, np.complex128),
                     _ffi.DeviceArray(nrow, np.float64))
    for sigma, expect in ((0.0, np.zeros(nrow, dtype=np.int64)), (of.LOOP_SIGMA, want)):
        _ffi.random_bits_rows_dev(bits, nb, nrow, of.LOOP_SEED)
        _ffi.gray_map_rows_dev(bits.ptr, nb, nq, nrow, _ffi.QAM, of.LOOP_MOD, np.complex128, sym.ptr)
        _ffi.ofdm_tx_rows_dev(sym, tx, of.LOOP_SYMS, nrow, of.LOOP_NF, of.LOOP_NC, 0, True, of.LOOP_NCP)
        _ffi.awgn_rows_dev(tx, tx, nt, nrow, of.LOOP_SEED + 1, g=1.0, sigma=sigma)
        _ffi.ofdm_rx_rows_dev(tx, z, of.LOOP_SYMS, nrow, of.LOOP_NF, of.LOOP_NC, 0, True, of.LOOP_NCP)
        _ffi.qam_scale_rows_dev(z.ptr, nq, 0, 1, nq, nrow, np.complex128, of.LOOP_MOD, r.ptr)
        _ffi.gray_demap_rows_dev(z.ptr, nq, 0, 1, nq, nrow, np.complex128, _ffi.QAM, of.LOOP_MOD, rx.ptr, r_ptr=r.ptr)
        _ffi.bit_count_rows_dev(bits.ptr, nb, rx.ptr, nb, nb, nrow, False, cnt.ptr)
        counts = cnt.read().view(np.int64)
        print("sigma %.2f: %s errors of %d bits per row" % (sigma, counts.tolist(), nb))
        assert np.array_equal(counts, expect)
    for d in (bits, rx, cnt, sym, tx, z, r):
        d.free()
