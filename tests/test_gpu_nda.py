"""Symbol timing recovery over frame sets on the GPU (csrc/timing.hip): the device against the NumPy host form bit for bit, across lane masks, partial
waves, the loop's first iterations, tile edges, strided rows and strided outputs; the outputs inside guard bands, with nothing written behind a row's
count; the input window alone is read; the overflow of max_symbols; a NaN sample; the golden cases of the reference within the bound of
tests/test_nda_cpu.py; and matched filter -> timing loop -> carrier loop end to end.  DESIGN.md 4.23."""
import json
import os

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dcm, sigsys as ss, synchronization as sync
from conftest import ROOT
from _pads import loud

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "g28_nda.npz"))
CASES = json.loads(str(G["cases"]))
NAMES = _ffi.NDA_OUTPUTS
T = 16                                   # the kernel's tile length in loop iterations (tests/test_nda_cpu.py pins it to the plan)
ROWS = (1, 63, 64, 65, 130)
PAD = GUARD = 40
A_STD = 3e-15


@pytest.fixture(scope="module", autouse=True)
def _device():
    _ffi.init(0)


def frames(rng, nrow, n, Ns, dt=np.complex128, sigma=0.05):
    """QPSK through a triangular pulse of two symbols, a different timing phase per row, plus noise"""
    nsym = n // Ns + 3
    s = (2 * rng.integers(0, 2, (nrow, nsym)) - 1) + 1j * (2 * rng.integers(0, 2, (nrow, nsym)) - 1)
    t = (np.arange(n)[None, :] + rng.uniform(0, Ns, (nrow, 1))) / Ns
    k = t.astype(int)
    x = np.take_along_axis(s, k, 1) * (1 - (t - k)) + np.take_along_axis(s, k + 1, 1) * (t - k)
    return (x + sigma * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))).astype(dt)


def lengths_for(Ns):
    first = Ns * Ns - Ns
    return [0, 1, first - 1, first, T - 1, T, T + 1, 3 * T + 5] + [first + j for j in (T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)]


def fill_of(kind, count, dt, first=0):
    if kind == "zeros":
        return np.zeros(count, dtype=dt)
    if kind == "nan":
        return np.full(count, np.nan + 1j * np.nan if np.dtype(dt).kind == "c" else np.nan, dtype=dt)
    return loud(count, dt, first)


def dev_rows(z, Ns, L, BnTs, I_ord=3, start=0, normalize=True, cap=None, outputs=NAMES, fill="loud", mark="loud", x_extra=0, y_extra=0):
    """NDA_symb_sync_rows' kernels on device buffers laid out by the test: row r's frame sits at start of rows x_stride apart, every other element of
    the input buffer -- pads in front and behind, the `start` elements and the gaps between rows -- holds `fill`.  The outputs lie y_stride apart between
    guard bands of `mark` values; what the call must not write -- the bands, the gaps, and everything behind min(counts[row], cap) elements of a row -- is
    checked here.  Returns (zz, e_tau, counts), zero behind the counts, None for an output that was not selected."""
    nrow, n = z.shape
    dt = z.dtype
    cap = _ffi.nda_iters(n, Ns) if cap is None else cap
    xs, ys = start + n + x_extra, cap + y_extra
    body = (nrow - 1) * xs + start + n if nrow else 0
    host = fill_of(fill, 2 * PAD + body + 1, dt)
    for r in range(nrow):
        host[PAD + r * xs + start:PAD + r * xs + start + n] = z[r]
    xbuf = _ffi.DeviceArray.from_host(host)
    xw = xbuf.window(PAD, body + 1)
    k1, k2, gains = _ffi.nda_gains_rows(BnTs, 0.707, Ns, nrow)
    gd = None if gains is None else _ffi.DeviceArray.from_host(gains.reshape(-1))
    cd = _ffi.device_bytes_of(np.full(max(nrow, 1), -7, dtype=np.int64))
    block = (nrow - 1) * ys + cap if nrow and cap else 0
    dts = dict(zz=dt, e_tau=np.float64)
    marks = {o: fill_of(mark, 2 * GUARD + block + 1, dts[o], 7) for o in outputs}
    bufs = {o: _ffi.DeviceArray.from_host(marks[o]) for o in outputs}
    win = {o: (bufs[o].window(GUARD, block + 1) if o in outputs else None) for o in NAMES}
    _ffi.nda_rows_dev(xw, n, nrow, Ns, L, I_ord, k1, k2, cap, cd, win["zz"], win["e_tau"], gd, xs, ys, start, normalize, dt)
    _ffi.sync()
    counts = cd.read().view(np.int64)[:nrow].copy()
    got = {o: None for o in NAMES}
    for o in outputs:
        back = bufs[o].to_host()
        keep = np.ones(back.size, dtype=bool)
        out = np.zeros((nrow, cap), dtype=dts[o])
        for r in range(nrow if cap else 0):
            k = min(int(counts[r]), cap)
            keep[GUARD + r * ys:GUARD + r * ys + k] = False
            out[r, :k] = back[GUARD + r * ys:GUARD + r * ys + k]
        assert np.array_equal(back[keep], marks[o][keep], equal_nan=True), "%s: written outside its rows' counts" % o
        got[o] = out
    for d in [xbuf, gd, cd] + list(bufs.values()):
        if d is not None:
            d.free()
    return got["zz"], got["e_tau"], counts


def same(got, want, what):
    for name, g, w in zip(NAMES + ("counts",), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, name)


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("Ns", [2, 3, 4, 8, 16])
def test_every_length_row_count_and_order_equals_the_host_form(Ns):
    rng = np.random.default_rng(2810 + Ns)
    for i, n in enumerate(lengths_for(Ns)):
        i += Ns
        I_ord, L, nrow = 1 + i % 3, (0, 2, 8)[(i // 3) % 3], ROWS[i % 5]
        dt = (np.complex128, np.complex64)[(i // 2) % 2]
        if _ffi.nda_refused_length(n, Ns, I_ord):
            n += 1
        start = (0, 5, 3)[i % 3]
        z = frames(rng, nrow, n, Ns, dt)
        bn = 0.02 if i % 4 else rng.uniform(0.005, 0.1, nrow)
        normalize = i % 3 != 1
        want = sync.NDA_symb_sync_rows_host(z, Ns, L, bn, I_ord=I_ord, normalize=normalize)
        got = dev_rows(z, Ns, L, bn, I_ord, start, normalize, x_extra=i % 4, y_extra=i % 3)
        same(got, want, (Ns, n, I_ord, L, nrow, dt, start))
        wide = np.concatenate([np.full((nrow, start), 99, dtype=dt), z], axis=1)
        same(sync.NDA_symb_sync_rows(wide, Ns, L, bn, I_ord=I_ord, start=start, normalize=normalize), want, ("public", Ns, n, I_ord, L, nrow, dt))


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_the_device_reads_only_its_input_window_and_writes_only_up_to_the_counts(dt):
    """pads, the elements in front of `start` and between the rows: zeros, loud values or NaNs there change nothing; the output block starts as NaN in the
    second run, and nothing behind a row's count is written (dev_rows checks it)"""
    z = frames(np.random.default_rng(2820), 65, 3 * T + 21, 4, dt)
    runs = [dev_rows(z, 4, 2, 0.02, 3, start=5, fill=f, mark=m, x_extra=9, y_extra=2) for f, m in (("zeros", "loud"), ("loud", "loud"), ("nan", "nan"))]
    for other in runs[1:]:
        same(other, runs[0], "fill")
    assert not any(np.any(np.isnan(v)) for v in runs[0][:2])
    same(runs[0], sync.NDA_symb_sync_rows_host(z, 4, 2, 0.02), "host")


def test_rows_driven_out_of_lock_equal_the_host_form():
    rng = np.random.default_rng(2821)
    z = frames(rng, 130, 3 * T + 30, 4)
    bn = rng.uniform(4.0, 12.0, 130)
    want = sync.NDA_symb_sync_rows_host(z, 4, 2, bn)
    assert want[2].max() >= _ffi.nda_iters(z.shape[1], 4) - 4 and want[2].min() <= 2          # W above 1 for good in one row, below 0 in another
    same(dev_rows(z, 4, 2, bn, y_extra=1), want, "unlocked")


# ---------------------------------------------------------------------------------------------------------------- outputs and overflow
def test_every_subset_of_the_outputs_gives_the_same_bits():
    z = frames(np.random.default_rng(2822), 65, 2 * T + 19, 3, np.complex64)
    for normalize in (True, False):
        full = dev_rows(z, 3, 1, 0.02, 2, normalize=normalize, y_extra=1)
        same(full, sync.NDA_symb_sync_rows_host(z, 3, 1, 0.02, I_ord=2, normalize=normalize), "full")
        for outs in (("zz",), ("e_tau",), ("e_tau", "zz")):
            got = dev_rows(z, 3, 1, 0.02, 2, normalize=normalize, outputs=outs, y_extra=1)
            assert np.array_equal(got[2], full[2]) and all(np.array_equal(got[NAMES.index(o)], full[NAMES.index(o)], equal_nan=True) for o in outs), outs
            pub = sync.NDA_symb_sync_rows(z, 3, 1, 0.02, I_ord=2, normalize=normalize, outputs=outs)
            assert len(pub) == len(outs) + 1 and all(np.array_equal(p, full[NAMES.index(o)], equal_nan=True) for p, o in zip(pub, outs)) and np.array_equal(pub[-1], full[2])


def test_max_symbols_overflow_raises_and_leaves_the_guard_bands_intact():
    z = frames(np.random.default_rng(2823), 65, 4 * T + 3, 4)
    full = sync.NDA_symb_sync_rows_host(z, 4, 2, 0.02, normalize=False)
    cap = int(full[2].min()) - 2
    zz, e, counts = dev_rows(z, 4, 2, 0.02, normalize=False, cap=cap, y_extra=1)            # (dev_rows checks the bands and the gaps)
    assert np.array_equal(counts, full[2]) and np.array_equal(zz, full[0][:, :cap]) and np.array_equal(e, full[1][:, :cap])
    with pytest.raises(ValueError, match="rows"):
        sync.NDA_symb_sync_rows(z, 4, 2, 0.02, max_symbols=cap)
    ok = sync.NDA_symb_sync_rows(z, 4, 2, 0.02, normalize=False, max_symbols=int(full[2].max()))
    assert ok[0].shape == (65, full[2].max()) and np.array_equal(ok[0], full[0][:, :full[2].max()])


def test_a_nan_sample_leaves_every_other_row_bit_identical():
    z = frames(np.random.default_rng(2824), 65, 3 * T + 9, 4)
    clean = sync.NDA_symb_sync_rows(z, 4, 2, 0.02)
    z[17, T + 3] = np.nan
    got = sync.NDA_symb_sync_rows(z, 4, 2, 0.02)
    same(got, sync.NDA_symb_sync_rows_host(z, 4, 2, 0.02), "nan")
    assert got[2][17] < clean[2][17] and all(np.array_equal(np.delete(g, 17, 0), np.delete(c, 17, 0)) for g, c in zip(got, clean))


def test_one_row_calls_and_real_input():
    z = frames(np.random.default_rng(2825), 2, 90, 4)
    for one, host in ((sync.NDA_symb_sync(z[0], 4, 2, 0.02, I_ord=2), sync.NDA_symb_sync_host(z[0], 4, 2, 0.02, I_ord=2)),
                      (sync.NDA_symb_sync(z[1].real.astype(np.float32), 4, 0, 0.05), sync.NDA_symb_sync_host(z[1].real.astype(np.float32), 4, 0, 0.05))):
        assert one[0].dtype == host[0].dtype and np.array_equal(one[0], host[0]) and np.array_equal(one[1], host[1]) and one[0].size > 15
    with pytest.raises(ValueError):
        sync.NDA_symb_sync(z[0, :9], 2, 1, 0.02, I_ord=2)
    with pytest.raises(ValueError):
        sync.NDA_symb_sync(z[0], 4, 9, 0.02)


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_golden_cases_meet_the_bound_of_the_host_form():
    for c in CASES:
        k = c["key"]
        z = G[c["signal"]]
        z = z[:z.size - c["trim"]].reshape(1, -1)
        raw, e, counts = sync.NDA_symb_sync_rows(z, c["Ns"], c["L"], c["BnTs"], c["zeta"], c["I_ord"], normalize=False)
        n = int(counts[0])
        assert n == G[k + "_e_tau"].size, k
        zz = sync.NDA_symb_sync(z[0], c["Ns"], c["L"], c["BnTs"], c["zeta"], c["I_ord"])[0]
        bound, bound_n = 16 * c["S"], (16 * c["S"] + A_STD * np.max(np.abs(G[k + "_raw"]))) / c["std"]
        errs = (np.max(np.abs(raw[0, :n] - G[k + "_raw"])), np.max(np.abs(e[0, :n] - G[k + "_e_tau"])), np.max(np.abs(zz - G[k + "_zz"])))
        print("%s: raw zz %.2e e_tau %.2e bound %.2e | zz %.2e bound %.2e" % (k, errs[0], errs[1], bound, errs[2], bound_n))
        assert max(errs[:2]) <= bound and errs[2] <= bound_n, (k, errs, bound, bound_n)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_matched_filter_timing_loop_and_carrier_loop_equal_the_chain_of_host_forms():
    """bits -> mpsk_gray_encode_bb_rows (ns = 4) -> a different timing phase per row (time_step_rows) -> matched_filter_rows at the sample rate ->
    NDA_symb_sync_rows(normalize=False) -> DD_carrier_sync_rows over the first counts.min() symbols, on 130 rows of 64 QPSK symbols"""
    ns, nrow, nsym = 4, 130, 64
    bits = np.random.default_rng(2826).integers(0, 2, (nrow, 2 * nsym)).astype(np.uint8)
    x_dev, b = dcm.mpsk_gray_encode_bb_rows(bits, ns, 4, 'src')
    x_host, _ = dcm.mpsk_gray_encode_bb_rows_host(bits, ns, 4, 'src')
    assert np.array_equal(x_dev, x_host)
    shifts = np.arange(nrow) % ns
    s_dev, s_host = sync.time_step_rows(x_dev, ns, shifts, 0), sync.time_step_rows_host(x_host, ns, shifts, 0)
    assert np.array_equal(s_dev, s_host)
    m_dev, m_host = ss.matched_filter_rows(s_dev, b, 0, 1), ss.matched_filter_rows_host(s_host, b, 0, 1)
    assert np.array_equal(m_dev, m_host)
    t_dev, t_host = sync.NDA_symb_sync_rows(m_dev, ns, 2, 0.02, normalize=False), sync.NDA_symb_sync_rows_host(m_host, ns, 2, 0.02, normalize=False)
    same(t_dev, t_host, "timing")
    k = int(t_dev[2].min())
    assert k > nsym - 16
    c_dev = sync.DD_carrier_sync_rows(np.ascontiguousarray(t_dev[0][:, :k]), 4, 0.05)
    c_host = sync.DD_carrier_sync_rows_host(np.ascontiguousarray(t_host[0][:, :k]), 4, 0.05)
    assert all(np.array_equal(a, h, equal_nan=True) for a, h in zip(c_dev, c_host))
    # the loop finds each row's timing phase: behind the pull-in the interpolants sit on the QPSK points' scale
    tail = np.abs(t_dev[0][:, k - 12:k])
    assert np.median(np.abs(tail - np.median(tail))) < 0.2 * np.median(tail)
