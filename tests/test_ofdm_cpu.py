"""OFDM without a GPU: mux_pilot_blocks and the _host restatements of ofdm_tx / ofdm_rx / chan_est_equalize against every result captured from
the real reference (tests/golden/gen_golden_ofdm.py -> g24_ofdm.npz, g24_conventions.json), the estimator's documented intent on a dispersive
channel, the argument conventions, and the kernels' per-thread phases walked thread by thread on the CPU (tests/host/ofdm_emul.cpp, every global
access checked against the row's window and its alignment), once more under -fsanitize=address,undefined as a stand-alone program.
Bounds: DESIGN.md 4.19."""
import logging
import os
import subprocess

import numpy as np
import pytest
from scipy import signal

from sk_dsp_comm_amd import _ffi, digitalcom as dc
from conftest import ROOT
import _ofdm as of

CODES = {np.dtype(np.complex64): 1, np.dtype(np.complex128): 3}


# ---------------------------------------------------------------------------------------------------------------- the reference's results
def test_fixture_covers_what_the_issue_lists():
    g, mux, cases = of.g24()
    shapes = {(c["symbols"], c["nf"], c["nc"], c["npb"], c["cp"], c["ncp"]) for c in cases}
    assert {(100, 32, 64, 10, True, 8), (99, 32, 64, 10, True, 8), (7, 2, 64, 2, True, 64), (8, 62, 64, 3, True, 1), (5, 30, 128, 0, False, 7),
            (9, 100, 256, 4, True, 0)} <= shapes and len(shapes) == 10 and any(s[0] == 0 for s in shapes)
    assert {m["mode"] for c in cases for m in c["rx"]} == {"none", "ideal", "pilot"}
    divisible = {m["N"] % (m["npb"] - 1) == 0 for m in mux}
    assert divisible == {True, False} and any(0 < m["N"] < m["npb"] - 1 for m in mux) and any(m["N"] == 0 for m in mux)
    assert np.array_equal(g["hc"], of.HC) and np.min(np.abs(np.fft.fft(of.HC, 4096))) >= 0.45
    conv = of.conv24()
    assert {"no_print_no_plots", "dtype", "estimator_intent", "value_errors", "empty_input"} <= set(conv["deliberate_differences"])
    assert conv["reference_behaviour"]["ofdm_rx(npb > 0, ht=None)"] == "AxisError" and conv["reference_behaviour"]["ofdm_tx(npb = 1)"] == "ZeroDivisionError"


def test_signatures_are_the_reference_s():
    import inspect
    for name, sig in of.conv24()["signatures"].items():
        assert str(inspect.signature(getattr(dc, name))) == sig, name


def test_mux_pilot_blocks_equals_the_reference_exactly():
    g, mux, _ = of.g24()
    for m in mux:
        y, ref = dc.mux_pilot_blocks(g[m["key"] + "_d"], m["npb"]), g[m["key"] + "_y"]
        assert y.dtype == ref.dtype == np.complex128 and y.shape == ref.shape and np.array_equal(y, ref), m
        if m["N"] % (m["npb"] - 1) == 0:
            assert not np.any(y[-1])            # the reference's trailing row of zeros
    with pytest.raises(ValueError):
        dc.mux_pilot_blocks(np.ones((4, 2)), 1)


def test_host_forms_equal_the_reference(caplog):
    g, _, cases = of.g24()
    for case in cases:
        with caplog.at_level(logging.INFO, logger=dc.__name__):
            caplog.clear()
            e = max(of.check_case_tx(g, case, dc.ofdm_tx_host), of.check_case_rx(g, case, dc.ofdm_rx_host))
        print("%s: %.2e" % (case["key"], e))
    case = [c for c in cases if c["nc"] == 96][0]        # an nc the kernels do not take: the public functions route it to the host, logged
    with caplog.at_level(logging.INFO, logger=dc.__name__):
        caplog.clear()
        of.check_case_tx(g, case, dc.ofdm_tx)
        of.check_case_rx(g, case, dc.ofdm_rx)
    assert sum("host float64 path" in r.getMessage() for r in caplog.records) == 1 + len(case["rx"])


def test_single_precision_in_gives_single_precision_out():
    g, _, cases = of.g24()
    case = cases[3]
    data = g[case["key"] + "_data"]
    for x in (data.astype(np.complex64), data.real.astype(np.float32)):
        y = dc.ofdm_tx_host(x, case["nf"], case["nc"], case["npb"], case["cp"], case["ncp"])
        assert y.dtype == np.complex64
    of.close(dc.ofdm_tx_host(data.astype(np.complex64), case["nf"], case["nc"], case["npb"], case["cp"], case["ncp"]), g[case["key"] + "_tx"])
    z, H = dc.ofdm_rx_host(of.rx_input(g, case).astype(np.complex64), case["nf"], case["nc"], -1, case["cp"], case["ncp"], ht=of.HC)
    assert z.dtype == np.complex64 and H.dtype == np.complex128
    assert dc.ofdm_tx_host(np.arange(64), 32, 64).dtype == np.complex128


def test_estimator_intent_recovers_the_data_through_a_dispersive_channel():
    """ht=None: tx -> lfilter(hc) -> rx divides each data symbol by the estimate of the latest pilot in front of it.  The channel is constant and
    shorter than the prefix, so every pilot equals the channel on its carriers and the data come back to 1e-12 / 0.45 at alpha = 0.9 (2e-15
    measured with the NumPy restatement)."""
    rng = np.random.default_rng(241)
    for symbols, npb in ((45, 10), (40, 10), (7, 2)):
        data = of.qam16(rng, symbols * 32)
        c = signal.lfilter(of.HC, 1, dc.ofdm_tx_host(data, 32, 64, npb, True, 8))
        z, H = dc.ofdm_rx_host(c, 32, 64, npb, True, 8, alpha=0.9)
        n = min(z.size, data.size)
        assert n == data.size
        err = float(np.max(np.abs(z[:n] - data)))
        print("%d symbols, npb %d: %.2e" % (symbols, npb, err))
        assert err <= 1e-12 * float(np.max(np.abs(data))) / 0.45
        Hht = np.fft.fft(of.HC, 64)
        if symbols % (npb - 1):                                                # (else the trailing zero row is a "pilot" and scales H by alpha)
            of.close(H, np.hstack((Hht[1:17], Hht[48:])), "H")
        else:
            of.close(H, 0.9 * np.hstack((Hht[1:17], Hht[48:])), "H")


def test_chan_est_equalize_host_is_the_reference_s_recursion():
    rng = np.random.default_rng(242)
    z = rng.standard_normal((11, 6)) + 1j * rng.standard_normal((11, 6))
    ht = rng.standard_normal(6) + 1j * rng.standard_normal(6) + 3
    for npb in (2, 3, 5, 11, 12):
        H, k_fill, want = None, 0, np.zeros_like(z)
        for k in range(11):
            if k % npb == 0:
                H = z[k] if k == 0 else 0.8 * H + (1 - 0.8) * z[k]
            else:
                want[k_fill] = z[k] / ht
                k_fill += 1
        zz, Hh = dc.chan_est_equalize_host(z, npb, 0.8, ht)
        assert np.array_equal(zz, want[:k_fill]) and np.array_equal(Hh, H)
        zi, _ = dc.chan_est_equalize_host(z, npb, 0.8)
        assert zi.shape == zz.shape


def test_convention_errors():
    x = np.ones(640, dtype=np.complex128)
    for fn in (dc.ofdm_tx, dc.ofdm_tx_host):
        for args in ((31, 64), (64, 64), (63, 64), (0, 64), (32, 64, 1), (32, 64, -1), (32, 64, 0, True, 65), (32, 64, 0, True, -1), (32, 96, 1)):
            with pytest.raises(ValueError):
                fn(x, *args)
    for fn in (dc.ofdm_rx, dc.ofdm_rx_host):
        for args, kw in (((31, 64), {}), ((64, 64), {}), ((32, 64, 1), {}), ((32, 64, -2), {}), ((32, 64, 0, True, 65), {}), ((32, 64, 0, True, -1), {}),
                         ((32, 64, -1), {}), ((32, 64, -1), {"ht": np.ones(65)}), ((32, 64, 2), {"ht": np.ones(65)})):
            with pytest.raises(ValueError):
                fn(x, *args, **kw)
    for fn in (dc.chan_est_equalize, dc.chan_est_equalize_host):
        with pytest.raises(ValueError):
            fn(np.ones((4, 2), dtype=complex), 1, 0.9)
    L = _ffi.load()
    for nc in (32, 96, 8192):
        assert L.skdsp_ofdm_tx_rows_dev(None, 0, 0, 0, 3, 2, nc, 0, 0, 0, None, 0) == -1          # SKDSP_ERR_BADARG without a device
        assert L.skdsp_ofdm_rx_rows_dev(None, 0, 0, 0, 3, 2, nc, 0, 0, 0, 0.9, None, None, 0, None) == -1
    assert L.skdsp_ofdm_tx_rows_dev(None, 0, 0, 0, 3, 2, 64, 0, 0, 0, None, 0) == 0
    assert L.skdsp_ofdm_tx_rows_dev(None, 0, 0, 0, 3, 3, 64, 0, 0, 0, None, 0) == -1
    assert L.skdsp_ofdm_rx_rows_dev(None, 0, 0, 0, 3, 2, 64, -1, 0, 0, 0.9, None, None, 0, None) == -1
    assert L.skdsp_ofdm_equalize_rows_dev(None, 0, 0, 0, 3, 2, 1, 0.9, None, None, 0, None) == -1


def test_empty_and_short_inputs():
    for fn in (dc.ofdm_tx, dc.ofdm_tx_host):
        for dt in (np.complex128, np.complex64):
            y = fn(np.ones(31, dtype=dt), 32, 64, 0, True, 8)
            assert y.shape == (0,) and y.dtype == dt
    for fn in (dc.ofdm_rx, dc.ofdm_rx_host):
        z, H = fn(np.ones(71, dtype=np.complex64), 32, 64, 0, True, 8)
        assert z.shape == (0,) and z.dtype == np.complex64 and np.array_equal(H, np.ones(32)) and H.dtype == np.float64
        z, H = fn(np.zeros(0), 32, 64, -1, True, 8, ht=of.HC)
        Hht = np.fft.fft(of.HC, 64)
        assert z.shape == (0,) and z.dtype == np.complex128 and np.array_equal(H, np.hstack((Hht[1:17], Hht[48:])))
        z, H = fn(np.zeros(5), 32, 64, 3, True, 8)
        assert z.shape == (0,) and H.shape == (32,) and np.all(np.isnan(H))
    assert dc.ofdm_tx_rows(np.zeros((0, 64)), 32, 64).shape == (0, 128) and dc.ofdm_rx_rows(np.zeros((3, 10)), 32, 64)[0].shape == (3, 0)


# ---------------------------------------------------------------------------------------------------------------- the emulated kernels
def build_emul(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "ofdm_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("ofdm"), "ofdm_emul", [])


def strided(x2d, off):
    """`off` elements, then the rows n + 1 elements apart: exactly off + (nrow - 1) (n + 1) + n elements; the emulation reads from element off on"""
    nrow, n = x2d.shape
    buf = np.zeros((nrow - 1) * (n + 1) + n, dtype=x2d.dtype)
    for r in range(nrow):
        buf[r * (n + 1):r * (n + 1) + n] = x2d[r]
    return buf


def unstrided(f, dtype, off, n, nrow):
    """the rows of an emulated output allocation; every other byte of it must still be the 0xEE fill"""
    raw = np.fromfile(f, dtype=np.uint8)
    esz = np.dtype(dtype).itemsize
    own = np.zeros(raw.size, dtype=bool)
    for r in range(nrow):
        own[(off + r * (n + 1)) * esz:(off + r * (n + 1) + n) * esz] = True
    assert raw.size == (off + (nrow - 1) * (n + 1) + n) * esz and np.all(raw[~own] == 0xEE), "a byte outside the rows was written"
    el = raw.view(dtype)
    return np.stack([el[off + r * (n + 1):off + r * (n + 1) + n] for r in range(nrow)])


def emul_tx(exe, tmp, x2d, nf, nc, npb, cp, ncp, xoff=0, yoff=0):
    nrow, nsym = x2d.shape[0], x2d.shape[1] // nf
    f = [os.path.join(str(tmp), v) for v in ("x.bin", "y.bin")]
    strided(x2d, xoff).tofile(f[0])
    subprocess.check_call([exe, "tx", str(CODES[x2d.dtype]), str(nsym), str(nrow), str(nf), str(nc), str(npb), str(int(cp)), str(ncp), str(xoff), str(yoff)] + f,
                          stdout=subprocess.DEVNULL)
    return unstrided(f[1], x2d.dtype, yoff, _ffi.ofdm_tx_symbols(nsym, npb) * (nc + (ncp if cp else 0)), nrow)


def emul_rx(exe, tmp, x2d, nsym, nf, nc, npb, cp, ncp, alpha, hht, xoff=0, zoff=0):
    nrow = x2d.shape[0]
    f = [os.path.join(str(tmp), v) for v in ("x.bin", "hht.f64", "z.bin", "h.bin")]
    strided(x2d, xoff).tofile(f[0])
    (np.zeros(nf, dtype=np.complex128) if hht is None else hht.astype(np.complex128)).tofile(f[1])
    subprocess.check_call([exe, "rx", str(CODES[x2d.dtype]), str(nsym), str(nrow), str(nf), str(nc), str(npb), str(int(cp)), str(ncp), repr(float(alpha)),
                           str(int(hht is not None)), str(xoff), str(zoff)] + f, stdout=subprocess.DEVNULL)
    return unstrided(f[2], x2d.dtype, zoff, _ffi.ofdm_rx_data_symbols(nsym, npb) * nf, nrow), np.fromfile(f[3], dtype=np.complex128).reshape(nrow, nf)


def emul_cases():
    """(nc, nf, symbols per row, npb, cp, ncp): both parities of log2 nc, NB > 1, R = 1, 2 and 4, symbol counts 1, NB - 1, NB, NB + 1"""
    out = []
    for i, nc in enumerate((64, 128, 512, 1024, 2048, 4096)):
        nb = max(1, 1024 // nc)
        for j, nsym in enumerate(sorted({1, nb - 1, nb, nb + 1} - {0})):
            nf = (2, nc // 2, nc - 2)[(i + j) % 3]
            npb = (0, 2, 3, 10)[(i + 2 * j) % 4]
            cp, ncp = ((True, 0), (True, 1), (True, 10), (True, nc), (False, 7))[(2 * i + j) % 5]
            out.append((nc, nf, nsym, npb, cp, ncp))
    return out


def run_emul_cases(exe, tmp, cases, dtypes, seed):
    rng = np.random.default_rng(seed)
    worst = 0.0
    for ci, (nc, nf, nsym, npb, cp, ncp) in enumerate(cases):
        for dt in dtypes:
            nrow = (1, 3)[ci % 2]
            off = ci % 2 if dt == np.complex64 else 0
            data = of.qam16(rng, (nrow, nsym * nf)).astype(dt)
            want = np.stack([dc.ofdm_tx_host(r, nf, nc, npb, cp, ncp) for r in data])
            got = emul_tx(exe, tmp, data, nf, nc, npb, cp, ncp, off, 1 - off if dt == np.complex64 else 0)
            worst = max(worst, of.close(got, want.astype(np.complex128), ("tx", nc, nf, nsym, npb, cp, ncp)))
            rx = np.stack([signal.lfilter(of.HC, 1, r) for r in want.astype(np.complex128)]).astype(dt)
            rsym = rx.shape[1] // (nc + ncp)
            if rsym == 0:
                continue
            used = rx[:, :rsym * (nc + ncp if cp else nc)]                   # what the kernel's rows hold: the reference ignores the rest
            Hht = np.fft.fft(of.HC, nc)
            hht = np.hstack((Hht[1:nf // 2 + 1], Hht[nc - nf // 2:]))
            for rnpb, ht in ((0, None), (-1, of.HC), (npb if npb else 3, of.HC), (npb if npb else 2, None)):
                ref = [dc.ofdm_rx_host(r.astype(np.complex128), nf, nc, rnpb, cp, ncp, 0.9, ht) for r in rx]
                z, h = emul_rx(exe, tmp, used, rsym, nf, nc, rnpb, cp, ncp, 0.9, None if ht is None else hht, 1 - off if dt == np.complex64 else 0, off)
                worst = max(worst, of.close(z, np.stack([r[0] for r in ref]), ("rx", nc, nf, rsym, rnpb, cp, ncp, ht is None), 1 / 0.45))
                if rnpb > 0:
                    of.close(h, np.stack([r[1] for r in ref]), ("H", nc, nf, rsym, rnpb))
    return worst


def test_pos_of_inverts_bin_of_and_the_geometry(emul):
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([emul, "pos"]).decode().splitlines()]
    assert rows == [(64, 16, 1), (128, 8, 1), (256, 4, 1), (512, 2, 1), (1024, 1, 1), (2048, 1, 2), (4096, 1, 4)]


def test_emulated_kernels_equal_the_host_forms(emul, tmp_path):
    """both kernels thread by thread, every global access checked against the row's window and its alignment: 1 and 3 rows, stride n + 1,
    complex64 windows on and one element off a 16-byte boundary, all four receiver modes"""
    worst = run_emul_cases(emul, tmp_path, emul_cases(), (np.complex128, np.complex64), 243)
    print("worst relative error of the emulated kernels (complex128 against 1e-12, complex64 against 2^-23): %.2e" % worst)


def test_emulated_chan_est_equalize_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(244)
    for dt in (np.complex128, np.complex64):
        for nsym, nf, npb, use_ht in ((11, 6, 3, False), (10, 300, 10, True), (7, 32, 2, False), (9, 2, 4, True), (1, 8, 5, False)):
            z = (rng.standard_normal((2, nsym, nf)) + 1j * rng.standard_normal((2, nsym, nf)) + 2).astype(dt)
            ht = rng.standard_normal(nf) + 1j * rng.standard_normal(nf) + 3 if use_ht else None
            f = [os.path.join(str(tmp_path), v) for v in ("z.bin", "hht.f64", "out.bin", "h.bin")]
            z.tofile(f[0])
            (np.zeros(nf, dtype=np.complex128) if ht is None else ht).tofile(f[1])
            subprocess.check_call([emul, "eq", str(CODES[np.dtype(dt)]), str(nsym), "2", str(nf), str(npb), "0.9", str(int(use_ht))] + f, stdout=subprocess.DEVNULL)
            ref = [dc.chan_est_equalize_host(r.astype(np.complex128), npb, 0.9, ht) for r in z]
            got = np.fromfile(f[2], dtype=dt).reshape(2, -1, nf)
            of.close(got, np.stack([r[0] for r in ref]), ("eq", nsym, nf, npb))
            of.close(np.fromfile(f[3], dtype=np.complex128).reshape(2, nf), np.stack([r[1] for r in ref]), ("eq H", nsym, nf, npb))


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process) over exact-size allocations"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "ofdm_emul_san", san)
    assert subprocess.call([exe, "pos"], stdout=subprocess.DEVNULL) == 0
    cases = [(64, 32, 17, 3, True, 8), (128, 126, 9, 0, False, 7), (1024, 2, 2, 2, True, 1024), (2048, 1024, 2, 0, True, 1), (4096, 4094, 1, 0, True, 10)]
    run_emul_cases(exe, tmp_path, cases, (np.complex64, np.complex128), 245)
