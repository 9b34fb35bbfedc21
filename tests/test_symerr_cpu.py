"""The symbol-error tools without a GPU: the NumPy host forms of xcorr / qam_sep / qpsk_bep / bpsk_bep against results captured from the real
reference (tests/golden/gen_golden_symerr.py -> g25_symerr.npz, g25_conventions.json), the exact-integer searches against the reference's
float-FFT searches, and both kernels walked thread by thread on the CPU (tests/host/symerr_emul.cpp) with every global and LDS access
bounds-checked, once more under -fsanitize=address,undefined as a stand-alone program.  Bounds: DESIGN.md 4.20.

xcorr's bound is the project's float64 parity figure, 1e-12 absolute on the energy-normalised correlation (|r| <= 1): a float64 direct sum lies
2e-17 from a long-double evaluation and the reference's FFT form 3.5e-16 (K = 4098).  Everything else is integers and compared exactly."""
import json
import logging
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc
from conftest import ROOT

CODES = {np.dtype(np.float32): 0, np.dtype(np.complex64): 1, np.dtype(np.float64): 2, np.dtype(np.complex128): 3}
G = np.load(os.path.join(ROOT, "tests", "golden", "g25_symerr.npz"))
CONV = json.load(open(os.path.join(ROOT, "tests", "golden", "g25_conventions.json")))
SEP, BPSK, QPSK, XC = (json.loads(str(G[k])) for k in ("sep", "bpsk", "qpsk", "xcorr"))


def sep_streams(c):
    t = G[c["key"] + "_tx"].astype(np.float64)
    return t[0] + 1j * t[1], G[c["key"] + "_rx"]


def logged(caplog, word):
    lines = [r.getMessage() for r in caplog.records if word in r.getMessage()]
    assert lines, "no log line with " + word
    return lines[-1]


# ---------------------------------------------------------------------------------------------------------------- fixtures
def test_fixture_covers_what_the_issue_lists():
    assert {c["mod"].lower() for c in SEP} == {"qpsk", "16qam", "64qam", "256qam"}
    assert {np.sign(c["taumax"]) for c in SEP} == {-1, 0, 1} and {c["kmax"] for c in SEP} == {0, 1, 2, 3}
    assert any(c["n_transient"] > 0 for c in SEP) and any(G[c["key"] + "_tx"].shape[1] != G[c["key"] + "_rx"].size for c in SEP)
    assert all(0.01 <= c["nerr"] / c["nsymb"] <= 0.20 for c in SEP)
    below = [2 * c["n_corr"] < min(G[c["key"] + "_tx"].shape[1], G[c["key"] + "_rx"].size) - c["n_transient"] for c in SEP]
    assert any(below) and not all(below)
    assert {(c["soft"], c["kmax"], int(np.sign(c["taumax"]))) for c in BPSK} >= {(False, 0, 1), (False, 1, -1), (True, 0, -1), (True, 1, 1)}
    kinds = {(G[c["key"] + "_x1"].dtype.kind, G[c["key"] + "_x1"].size % 2, 2 * c["n_lags"] >= G[c["key"] + "_x1"].size - 1) for c in XC}
    assert {(k, o) for k, o, _ in kinds} == {("f", 0), ("f", 1), ("c", 0), ("c", 1)} and {a for _, _, a in kinds} == {False, True}
    assert CONV["qpsk_bep_reference_raises"].startswith("TypeError") and CONV["numpy"]


# ---------------------------------------------------------------------------------------------------------------- host forms against the reference
@pytest.mark.parametrize("c", XC, ids=[c["key"] for c in XC])
def test_xcorr_host_equals_the_reference(c):
    r, k = dc.xcorr_host(G[c["key"] + "_x1"], G[c["key"] + "_x2"], c["n_lags"])
    assert r.dtype == np.complex128 and np.array_equal(k, G[c["key"] + "_k"])
    print("xcorr_host", c["key"], float(np.max(np.abs(r - G[c["key"] + "_r"]))))
    assert np.max(np.abs(r - G[c["key"] + "_r"])) <= 1e-12


@pytest.mark.parametrize("c", XC, ids=[c["key"] for c in XC])
def test_direct_lag_sums_equal_the_reference(c):
    """the direct float64 sum the kernel computes (here in NumPy), normalised, against the reference's FFT form"""
    R, k, E1, E2 = _ffi.lag_corr_host(G[c["key"] + "_x1"], G[c["key"] + "_x2"], c["n_lags"])
    assert np.array_equal(k, G[c["key"] + "_k"])
    assert np.max(np.abs(R / np.sqrt(E1 * E2) - G[c["key"] + "_r"])) <= 1e-12


def reference_form_sep_search(tx, rq, n_corr):
    """qam_sep's search as the reference writes it: four float xcorr calls, the maximum of the real parts"""
    Rs = [dc.xcorr_host(rq * (1j) ** k, tx, n_corr) for k in range(4)]
    tops = np.array([np.max(r.real) for r, _ in Rs])
    kmax = int(np.where(tops == tops.max())[0][0])
    r, lags = Rs[kmax]
    return kmax, int(lags[np.where(r.real == tops.max())[0]][0])


@pytest.mark.parametrize("c", SEP, ids=[c["key"] for c in SEP])
def test_qam_sep_host_equals_the_reference(c, caplog):
    tx, rx = sep_streams(c)
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        got = dc.qam_sep_host(tx, rx, c["mod"], c["n_corr"], c["n_transient"])
    assert got == (c["nsymb"], c["nerr"], c["nerr"] / float(c["nsymb"])) and [type(v) for v in got] == [int, int, float]
    assert logged(caplog, "Phase ambiquity") == 'Phase ambiquity = (1j)**%d, taumax = %d' % (c["kmax"], c["taumax"])
    assert logged(caplog, "Symbols") == 'Symbols = %d, Errors %d, SEP = %1.2e' % (c["nsymb"], c["nerr"], c["nerr"] / float(c["nsymb"]))
    # the exact-integer search against the float-FFT search of the reference, and against what was injected
    n = min(tx.size, rx.size) - c["n_transient"]
    t, rq = tx[c["n_transient"]:][:n], _ffi.qam_quantise_host(rx[c["n_transient"]:][:n], _ffi.QAM_LEVELS[c["mod"].lower()])
    assert dc.qam_sep_search(t, rq, c["n_corr"]) == reference_form_sep_search(t, rq, c["n_corr"]) == (c["kmax"], c["taumax"]) == (c["rot"], c["lag"])
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        dc.qam_sep_host(tx, rx, c["mod"], c["n_corr"], c["n_transient"], SEP_disp=False)
    assert not caplog.records


def test_quantiser_is_the_reference_expression_componentwise():
    rng = np.random.default_rng(25)
    x = 1.6 * (rng.standard_normal(4000) + 1j * rng.standard_normal(4000))
    x[:8] = [0.5 + 0.5j, -1 - 1j, 1 + 1j, 0, 1 / 3 - 1 / 3j, 5 - 5j, -0.0 + 0j, 1e300 - 1e300j]
    for M in (2, 4, 8, 16):
        q = np.rint((M - 1) * (x + (1 + 1j)) / 2.)
        q = np.clip(q.real, 0, M - 1) + 1j * np.clip(q.imag, 0, M - 1)
        assert np.array_equal(_ffi.qam_quantise_host(x, M), 2 * q - (M - 1) * (1 + 1j))


@pytest.mark.parametrize("c", BPSK, ids=[c["key"] for c in BPSK])
def test_bpsk_bep_host_equals_the_reference(c, caplog):
    tx, rx = G[c["key"] + "_tx"], G[c["key"] + "_rx"]
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        got = dc.bpsk_bep_host(tx, rx, c["n_corr"], c["n_transient"])
    assert got == (c["count"], c["errors"]) and type(got[0]) is int and isinstance(got[1], np.int64)
    assert logged(caplog, "kmax") == 'kmax =  %d, taumax = %d' % (c["kmax"], c["taumax"])
    heads = tx[c["n_transient"]:][:c["n_corr"]], rx[c["n_transient"]:][:c["n_corr"]]
    assert dc.bep_search(*heads, c["n_corr"], True) == dc.bep_search(*heads, c["n_corr"], True, exact=False) == (c["kmax"], c["taumax"])


def test_soft_bpsk_counts_are_the_reference_integers_not_zero_one():
    odd = 0
    for c in (c for c in BPSK if c["soft"]):
        tx, rx = G[c["key"] + "_tx"][c["n_transient"]:], G[c["key"] + "_rx"][c["n_transient"]:]
        t0, r0, count = dc._overlap(tx.size, rx.size, c["taumax"])
        sign = -1.0 if c["kmax"] else 1.0
        flags = np.int16((tx[t0:t0 + count] + 1) / 2) ^ np.int16((sign * rx[r0:r0 + count] + 1) / 2)
        assert np.sum(flags) == c["errors"]
        odd += np.count_nonzero((flags != 0) & (flags != 1))
    assert odd


def brute_qpsk(tx, rx, lag, rot):
    """an independent count at a known lag and rotation: Python integers, one symbol at a time"""
    t0, r0 = (-lag, 0) if lag < 0 else (0, lag)
    n = min(tx.size - t0, rx.size - r0)
    I = Q = S = 0
    for i in range(n):
        t, r = complex(tx[t0 + i]), complex(rx[r0 + i])
        for _ in range(rot):
            r = complex(-r.imag, r.real)
        eI, eQ = int((t.real + 1) / 2) ^ int((r.real + 1) / 2), int((t.imag + 1) / 2) ^ int((r.imag + 1) / 2)
        I, Q, S = I + eI, Q + eQ, S + (eI | eQ)
    return n, I, Q, S


@pytest.mark.parametrize("c", QPSK, ids=[c["key"] for c in QPSK])
def test_qpsk_bep_host_equals_the_brute_force_count(c, caplog):
    tx, rx = G[c["key"] + "_tx"], G[c["key"] + "_rx"]
    with caplog.at_level(logging.INFO, logger=dc.log.name):
        got = dc.qpsk_bep_host(tx, rx, c["n_corr"], c["n_transient"])
    assert logged(caplog, "kmax") == 'kmax =  %d, taumax = %d' % (c["rot"], c["lag"])
    assert got == brute_qpsk(tx[c["n_transient"]:], rx[c["n_transient"]:], c["lag"], c["rot"])
    assert type(got[0]) is int and all(isinstance(v, np.int64) for v in got[1:])
    heads = tx[c["n_transient"]:][:c["n_corr"]], rx[c["n_transient"]:][:c["n_corr"]]
    assert dc.bep_search(*heads, c["n_corr"]) == dc.bep_search(*heads, c["n_corr"], exact=False) == (c["rot"], c["lag"])


def test_conventions_that_need_no_device():
    tx, rx = sep_streams(SEP[0])
    with pytest.raises(ValueError, match="Unknown mod_type"):
        dc.qam_sep_host(tx, rx, "8psk")
    with pytest.raises(ValueError, match="Unknown mod_type"):
        dc.qam_sep(tx, rx, "8psk")
    bad = rx.copy()
    bad[5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        dc.qam_sep_host(tx, bad, "qpsk")
    with pytest.raises(ValueError, match="integer"):
        dc.qam_sep_host(tx + 0.25, rx, "qpsk")
    with pytest.raises(ValueError, match="zero energy"):
        dc.qam_sep_host(np.zeros(64), rx[:64], "qpsk")
    with pytest.raises(ValueError, match="zero energy"):
        dc.xcorr_host(np.zeros(10), np.ones(10), 3)
    with pytest.raises(ValueError):
        dc.xcorr_host(np.ones(10), np.ones(8), 3)
    with pytest.raises(ValueError, match="even"), pytest.warns(UserWarning):
        dc.qam_sep_host(tx, rx, "qpsk", n_corr=101)
    with pytest.raises(ValueError, match="65536"):
        dc.bpsk_bep_host(np.ones(8), np.ones(8), n_corr=2 ** 17)
    with pytest.raises(ValueError, match="finite"):
        dc.bpsk_bep_host(np.ones(8), np.array([1.0, np.inf] * 4))
    with pytest.raises(ValueError, match="int16"):
        dc.qpsk_bep_host(np.ones(8) + 1j, np.full(8, 1e6 + 1j))
    for fn in (_ffi.sym_count_rows_host, _ffi.sym_count_rows):          # the argument rules come before the library is touched
        with pytest.raises(ValueError):
            fn(np.ones((1, 4)), np.ones((1, 4)), 7)
        with pytest.raises(ValueError):
            fn(np.ones((1, 4)), np.ones((1, 4)), _ffi.SYM_QAM, 3)
        with pytest.raises(ValueError):
            fn(np.ones((1, 4)), np.ones((1, 4)), _ffi.SYM_BPSK, 0, 2)


def test_c_abi_argument_rules_need_no_device():
    L = _ffi.load()
    nl, l0 = _ffi.lag_corr_len(4099, 1024)
    assert (nl, l0) == (2049, -1024) and _ffi.lag_corr_len(301, 200) == (300, -150) and _ffi.lag_corr_len(1, 5) == (0, 0) and _ffi.lag_corr_len(64, 0) == (1, 0)
    assert L.skdsp_lag_corr_dev(None, 0, None, 0, 0, 4, 0, None, None) == 0 and L.skdsp_lag_corr(None, 0, None, 0, 1, 4, 0, None, None, None) == 0
    assert L.skdsp_lag_corr_dev(None, 9, None, 0, 8, 4, 0, None, None) == -1 and L.skdsp_lag_corr_dev(None, 0, None, 0, 8, 4, 3, None, None) == -1
    assert L.skdsp_lag_corr_dev(None, 0, None, 0, 8, -1, 0, None, None) == -1 and L.skdsp_lag_corr_dev(None, 0, None, 0, 8, 4, 0, None, None) == -1
    assert b"null pointer" in L.skdsp_last_error()
    cnt = lambda *a: L.skdsp_sym_count_rows_dev(None, a[0], 8, 0, None, 1, 8, 0, a[1], 0, a[2], a[3], a[4], a[5], a[6], None)
    assert cnt(1, 1, 4, 0, 0, 4, 0) == 0                                  # nrow = 0
    assert cnt(5, 1, 4, 1, 0, 4, 0) == -1 and cnt(1, 0, 4, 1, 0, 4, 0) == -1 and cnt(1, 1, -1, 1, 0, 4, 0) == -1
    assert cnt(1, 1, 4, 1, 3, 0, 0) == -1 and cnt(1, 1, 4, 1, 0, 5, 0) == -1 and cnt(1, 1, 4, 1, 2, 0, 2) == -1 and cnt(1, 1, 4, 1, 1, 0, 4) == -1
    counts = np.full(8, 7, dtype=np.int64)
    assert L.skdsp_sym_count_rows(None, 1, 0, 0, None, 1, 0, 0, 1, 0, 0, 2, 1, 0, 0, _ffi._ptr(counts)) == 0 and not counts.any()   # n = 0: zeros, no device


# ---------------------------------------------------------------------------------------------------------------- the emulation
def build_emul(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "symerr_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("symerr"), "symerr_emul", [])


def plan_of(exe):
    names = ("threads", "lags_wg", "tile", "win", "target_wgs", "max_parts", "sym_wg")
    return dict(zip(names, (int(w) for w in subprocess.check_output([exe, "plan"]).decode().split())))


def emul_lag(exe, tmp, a, b, n_lags, quant=0):
    """(R, E1, E2, plan words) of the emulated kernels; the files hold exactly the K elements a call reads"""
    K = 2 * (a.size // 2)
    fa, fb, fo = (os.path.join(str(tmp), f) for f in ("a.bin", "b.bin", "r.bin"))
    a[:K].tofile(fa)
    b[:K].tofile(fb)
    words = subprocess.check_output([exe, "lag", str(CODES[a.dtype]), str(CODES[b.dtype]), str(a.size), str(n_lags), str(quant), fa, fb, fo]).decode().split()
    out = np.fromfile(fo, dtype=np.float64)
    return out[:-2].view(np.complex128), out[-2], out[-1], dict(zip(("K", "nl", "ngroups", "nparts", "tpp", "l0"), (int(w) for w in words)))


def int_stream(rng, n, dt, top=15):
    v = rng.integers(-top, top + 1, n).astype(np.float64)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.integers(-top, top + 1, n)
    return v.astype(dt)


def exact_lag_sums(a, b, lags):
    """int64 evaluation of sum_n a[(n + l) mod K] conj(b[n]) for integer-valued streams"""
    ar, ai, br, bi = (np.rint(v).astype(np.int64) for v in (a.real, a.imag, b.real, b.imag))
    out = np.zeros((len(lags), 2), dtype=np.int64)
    for i, l in enumerate(lags):
        xr, xi = np.roll(ar, -int(l)), np.roll(ai, -int(l))
        out[i] = np.sum(xr * br + xi * bi), np.sum(xi * br - xr * bi)
    return out


def check_lag_exact(exe, tmp, a, b, n_lags, quant=0):
    R, E1, E2, plan = emul_lag(exe, tmp, a, b, n_lags, quant)
    K = plan["K"]
    lags = plan["l0"] + np.arange(plan["nl"])
    aq = _ffi.qam_quantise_host(a[:K], quant) if quant else a[:K].astype(np.complex128)
    want = exact_lag_sums(aq, b[:K].astype(np.complex128), lags)
    assert np.array_equal(R.real, want[:, 0]) and np.array_equal(R.imag, want[:, 1]), (K, n_lags)
    bq = b[:K].astype(np.complex128)
    assert E1 == np.sum(aq.real ** 2 + aq.imag ** 2) and E2 == np.sum(bq.real ** 2 + bq.imag ** 2)
    return plan


def test_plan_is_a_function_of_the_sizes_and_scratch_stays_bounded(emul):
    P = plan_of(emul)
    assert P["win"] == P["tile"] + P["lags_wg"] and P["tile"] % P["threads"] == 0
    for n, n_lags in ((2 ** 26, 1024), (2 ** 24, 1024), (2 ** 20, 1024), (2 ** 26, 0), (2 ** 20, 2 ** 19)):
        K, nl, ngroups, nparts, tpp, scratch = (int(w) for w in subprocess.check_output([emul, "lagplan", str(n), str(n_lags)]).decode().split())
        assert nparts <= P["max_parts"] and nparts * tpp >= -(-K // P["tile"]) > (nparts - 1) * tpp
        assert scratch * 8 <= 16 * (P["max_parts"] * max(ngroups, 1) * P["lags_wg"] + P["max_parts"])
        if nl <= 2049:
            assert scratch * 8 < 8 << 20                                  # megabytes at K = 2^26, not gigabytes


def test_emulated_lag_kernel_is_exact_on_integer_streams(emul, tmp_path):
    rng = np.random.default_rng(2501)
    P = plan_of(emul)
    G_, T = P["lags_wg"], P["tile"]
    # K = 2 (from an even and an odd length), n_lags = 0, below, at and above K / 2
    for n in (2, 3):
        for n_lags in (0, 1, 5):
            check_lag_exact(emul, tmp_path, int_stream(rng, n, np.complex128), int_stream(rng, n, np.complex128), n_lags)
    # a lag group at its constant and +- 1 (nl = 255, 257; 256 lags: all of K = 256), lags wrapping at both ends of the stream
    for n, n_lags, dt in ((1022, G_ // 2 - 1, np.complex64), (1022, G_ // 2, np.float64), (G_, G_, np.complex128), (G_ + 2, G_, np.float32), (1022, 300, np.complex128)):
        plan = check_lag_exact(emul, tmp_path, int_stream(rng, n, dt), int_stream(rng, n, np.complex128), n_lags)
        assert plan["ngroups"] == -(-plan["nl"] // G_)
    # a tile at its constant and +- 1 sample pair; n_lags >= K / 2 at more than one group
    for n, n_lags in ((T - 2, 7), (T, 7), (T + 2, 7), (T + 3, 1), (2 * G_ + 10, 10 ** 6)):
        check_lag_exact(emul, tmp_path, int_stream(rng, n, np.complex128), int_stream(rng, n, np.float64), n_lags)
    # a partition at its constant and +- 1 tile: one group, so the plan cuts at max_parts tiles
    for tiles in (P["max_parts"] - 1, P["max_parts"], P["max_parts"] + 1):
        plan = check_lag_exact(emul, tmp_path, int_stream(rng, tiles * T - 2, np.float32, 3), int_stream(rng, tiles * T - 2, np.float32, 3), 1)
        assert plan["nparts"] == (tiles if tiles <= P["max_parts"] else -(-tiles // 2)) and plan["tpp"] == (1 if tiles <= P["max_parts"] else 2)
    # the quantiser at the load: soft symbols against Gaussian integers
    for M in (2, 4, 8, 16):
        tx = (2 * rng.integers(0, M, 1500) - (M - 1)) + 1j * (2 * rng.integers(0, M, 1500) - (M - 1))
        soft = np.roll(tx, 4) / (M - 1) + 0.2 * (rng.standard_normal(1500) + 1j * rng.standard_normal(1500))
        check_lag_exact(emul, tmp_path, soft.astype(np.complex128), tx.astype(np.complex128), 20, M)
        check_lag_exact(emul, tmp_path, soft.astype(np.complex64), tx.astype(np.complex64), 20, M)


def test_emulated_lag_kernel_meets_the_float64_bound(emul, tmp_path):
    rng = np.random.default_rng(2502)
    for n, n_lags, dt in ((4098, 300, np.complex128), (4099, 3000, np.complex64), (1000, 50, np.float64), (2051, 7, np.float32)):
        cpx = np.dtype(dt).kind == "c"
        a = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cpx else 0)).astype(dt)
        b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cpx else 0)).astype(dt)
        R, E1, E2, plan = emul_lag(emul, tmp_path, a, b, n_lags)
        r, k = dc.xcorr_host(a, b, n_lags)
        assert np.array_equal(k, plan["l0"] + np.arange(plan["nl"]))
        print("emulated lag", n, n_lags, float(np.max(np.abs(R / np.sqrt(E1 * E2) - r))))
        assert np.max(np.abs(R / np.sqrt(E1 * E2) - r)) <= 1e-12


def emul_cnt(exe, tmp, tx, x, mode, levels, k, start, step, n, t0, r0):
    nrow = tx.shape[0]
    tx_el = (nrow - 1) * tx.shape[1] + t0 + n if n else 0
    x_el = (nrow - 1) * x.shape[1] + start + (r0 + n - 1) * step + 1 if n else 0
    ft, fx, fo = (os.path.join(str(tmp), f) for f in ("tx.bin", "x.bin", "c.bin"))
    tx.reshape(-1)[:tx_el].tofile(ft)
    x.reshape(-1)[:x_el].tofile(fx)
    subprocess.check_call([exe, "cnt", str(CODES[tx.dtype]), str(tx.shape[1]), str(t0), str(CODES[x.dtype]), str(x.shape[1]), str(start), str(step), str(r0), str(n),
                           str(nrow), str(mode), str(levels), str(k), ft, fx, fo])
    return np.fromfile(fo, dtype=np.int64).reshape(nrow, 4)


def count_case(rng, mode, M, nrow, n, t0, r0, start, step, tdt, xdt, spoil=False):
    """(tx, x): rows a little wider than what is read, symbols with errors, and (spoil) one of each precondition violation"""
    wt, wx = t0 + n + 2, start + (r0 + n) * step + 3
    if mode == _ffi.SYM_QAM:
        tx = (2 * rng.integers(0, M, (nrow, wt)) - (M - 1)) + 1j * (2 * rng.integers(0, M, (nrow, wt)) - (M - 1))
        scale = M - 1
    else:
        tx = (2 * rng.integers(0, 2, (nrow, wt)) - 1) + 1j * (2 * rng.integers(0, 2, (nrow, wt)) - 1)
        scale = 1
    x = 3.0 * (rng.standard_normal((nrow, wx)) + 1j * rng.standard_normal((nrow, wx)))
    idx = start + (r0 + np.arange(n)) * step
    x[:, idx] = tx[:, t0:t0 + n] / scale + (0.9 / scale) * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))
    if np.dtype(tdt).kind != "c":
        tx = tx.real
    if np.dtype(xdt).kind != "c":
        x = x.real
    tx, x = tx.astype(tdt), x.astype(xdt)
    if spoil and n >= 4:
        x[0, idx[0]] = np.nan
        x[-1, idx[n - 1]] = np.inf
        tx[0, t0 + 1] = 0.5 if mode == _ffi.SYM_QAM else 1e6
        x[-1, idx[2]] = -7e4
    return tx, x


COUNT_MODES = [(_ffi.SYM_QAM, M, k) for M in (2, 4, 8, 16) for k in range(4)] + [(_ffi.SYM_QPSK, 0, k) for k in range(4)] + [(_ffi.SYM_BPSK, 0, k) for k in range(2)]


def test_emulated_count_kernel_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(2503)
    W = plan_of(emul)["sym_wg"]
    sizes = (0, 1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1)
    dts = ((np.complex128, np.complex128), (np.complex64, np.complex64), (np.float64, np.complex64), (np.complex128, np.float32), (np.float32, np.float64))
    for i, (mode, M, k) in enumerate(COUNT_MODES):
        n, (tdt, xdt) = sizes[i % len(sizes)], dts[i % len(dts)]
        nrow, t0, r0, start, step = (1, 3)[i % 2], (0, 1, 5)[i % 3], (0, 3)[i % 2], (0, 2)[(i // 2) % 2], (1, 4)[(i // 3) % 2]
        tx, x = count_case(rng, mode, M, nrow, n, t0, r0, start, step, tdt, xdt, spoil=i % 4 == 1)
        want = _ffi.sym_count_rows_host(tx, x, mode, M, k, start, step, n, t0, r0)
        assert np.array_equal(emul_cnt(emul, tmp_path, tx, x, mode, M, k, start, step, n, t0, r0), want), (mode, M, k, n)
        assert n < 4 or want[:, :3].any()
    # every size at one mode each, and the soft QPSK integers that are neither 0 nor 1
    for n in sizes:
        for mode, M, k in ((_ffi.SYM_QAM, 4, 1), (_ffi.SYM_QPSK, 0, 3), (_ffi.SYM_BPSK, 0, 1)):
            tx, x = count_case(rng, mode, M, 3, n, 1, 3, 2, 4, np.complex128, np.complex128, spoil=True)
            want = _ffi.sym_count_rows_host(tx, x, mode, M, k, 2, 4, n, 1, 3)
            assert np.array_equal(emul_cnt(emul, tmp_path, tx, x, mode, M, k, 2, 4, n, 1, 3), want), (mode, n)
            assert n < 4 or (want[0, 3] == 2 and want[-1, 3] >= 1)


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process): both kernels over more than one group,
    tile, partition and work item, on inputs inside exact-size allocations"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "symerr_emul_san", san)
    rng = np.random.default_rng(2504)
    P = plan_of(exe)
    for n, n_lags, dt, M in ((2, 0, np.complex128, 0), (3, 9, np.float32, 0), (P["tile"] + 2, P["lags_wg"] // 2, np.complex64, 0), (2 * P["lags_wg"] + 10, 10 ** 6, np.float64, 0),
                             ((P["max_parts"] + 1) * P["tile"], 1, np.complex64, 0), (1500, 20, np.complex128, 16)):
        a = int_stream(rng, n, dt, 3) / (3.0 if M else 1.0)
        check_lag_exact(exe, tmp_path, a.astype(dt), int_stream(rng, n, dt, 3), n_lags, M)
    W = P["sym_wg"]
    for i, (mode, M, k) in enumerate(((_ffi.SYM_QAM, 16, 3), (_ffi.SYM_QPSK, 0, 1), (_ffi.SYM_BPSK, 0, 1))):
        for n, step in ((1, 1), (W + 1, 4), (2 * W + 1, 1)):
            tx, x = count_case(rng, mode, M, 3, n, 1, 3, 2, step, np.complex64, np.complex128, spoil=True)
            assert np.array_equal(emul_cnt(exe, tmp_path, tx, x, mode, M, k, 2, step, n, 1, 3), _ffi.sym_count_rows_host(tx, x, mode, M, k, 2, step, n, 1, 3))
