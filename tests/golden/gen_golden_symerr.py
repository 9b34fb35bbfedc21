#!/usr/bin/env python3
"""G25: the symbol-error tools -- digitalcom.xcorr (digitalcom.py:1163-1179), qam_sep (:495-582), qpsk_bep (:723-790), bpsk_bep (:793-846) --
results from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_symerr.py

  g25_symerr.npz        "xcorr": JSON list of {key, n_lags}: <key>_x1, <key>_x2 -> <key>_r, <key>_k.
                        "sep": JSON list of {key, mod, n_corr, n_transient, lag, rot, kmax, taumax, nsymb, nerr}: <key>_tx (int8 [2, n]: the
                        Gaussian integers of qam_bb's tx_data), <key>_rx (complex128); (kmax, taumax) are read from the reference's log line,
                        (lag, rot) are what the generator injected; sep is nerr / nsymb.
                        "bpsk": JSON list of {key, n_corr, n_transient, soft, kmax, taumax, count, errors}: <key>_tx, <key>_rx (float64).
                        "qpsk": JSON list of {key, n_corr, n_transient, lag, rot, soft}: <key>_tx, <key>_rx (complex128) -- inputs only: the
                        reference raises on every call (g25_conventions.json), the tests count by brute force at the injected lag and rotation.
  g25_conventions.json  signatures, the reference's TypeError in qpsk_bep and the NumPy version, the deliberate differences

Every input's correlation peak is unique: the generator evaluates the exact integer correlation (quantised rx against tx, or the two heads)
and REFUSES an input whose best candidate is attained twice, so no fixture depends on an FFT's rounding noise.  Every qam_sep case has
between 1 % and 20 % symbol errors.
"""
import inspect
import json
import logging
import os
import re
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SK_DSP_COMM_SRC", "/root/reference/src"))

import numpy as np  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402

rng = np.random.default_rng(2525)
out = {}
LEVELS = {'qpsk': 2, '16qam': 4, '64qam': 8, '256qam': 16}


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


_lines = _Lines()
dc.log.addHandler(_lines)
dc.log.setLevel(logging.INFO)


def logged(pattern):
    for line in reversed(_lines.lines):
        m = re.search(pattern, line)
        if m:
            return tuple(int(v) for v in m.groups())
    raise SystemExit("the reference did not log " + pattern)


def exact_circular(a, b):
    """sum_n a[(n + m) mod N] conj(b[n]) of small Gaussian integers, exactly (int64, direct)"""
    ar, ai, br, bi = (np.rint(v).astype(np.int64) for v in (a.real, a.imag, b.real, b.imag))
    N = a.size
    R = np.zeros((N, 2), dtype=np.int64)
    for m in range(N):
        xr, xi = np.roll(ar, -m), np.roll(ai, -m)
        R[m] = np.sum(xr * br + xi * bi), np.sum(xi * br - xr * bi)
    return R


def unique_peak(R, lags_kept, bpsk=False):
    """(k, lag) of the strictly largest candidate Re((1j)^k R), or SystemExit on a tie"""
    re_, im_ = R[lags_kept % R.shape[0], 0], R[lags_kept % R.shape[0], 1]
    cands = np.stack([re_, -re_] if bpsk else [re_, -im_, -re_, im_])
    top = cands.max()
    if np.count_nonzero(cands == top) != 1:
        raise SystemExit("refused: the exact correlation maximum is attained %d times" % np.count_nonzero(cands == top))
    k, i = np.unravel_index(np.argmax(cands), cands.shape)
    return int(k), int(lags_kept[i])


def quantise(rx, M):
    def comp(v):
        return 2 * np.clip(np.rint((M - 1) * (v + 1) / 2.), 0, M - 1) - (M - 1)
    return comp(rx.real) + 1j * comp(rx.imag)


def delayed(sym, lag, fill):
    """rx such that the reference aligns rx[lag:] with tx (lag >= 0) or rx with tx[-lag:] (lag < 0)"""
    return np.concatenate((fill[:lag], sym)) if lag >= 0 else sym[-lag:]


# ---------------------------------------------------------------------------------------------------------------- xcorr
xc = []
for key, n, cpx, n_lags in (("xc_real_even", 1000, False, 50), ("xc_real_odd_all", 1001, False, 600), ("xc_cpx_even", 4098, True, 1024),
                            ("xc_cpx_odd_all", 301, True, 200), ("xc_cpx_half", 300, True, 150), ("xc_cpx_zero", 64, True, 0)):
    x1 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cpx else 0)
    x2 = np.roll(x1, 3) * (0.8 - 0.3j if cpx else -0.7) + 0.5 * (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cpx else 0))
    r, k = dc.xcorr(x1, x2, n_lags)
    out[key + "_x1"], out[key + "_x2"], out[key + "_r"], out[key + "_k"] = x1, x2, np.asarray(r, dtype=np.complex128), np.asarray(k, dtype=np.int64)
    xc.append({"key": key, "n_lags": n_lags})
out["xcorr"] = json.dumps(xc)

# ---------------------------------------------------------------------------------------------------------------- qam_sep
sep = []
for key, mod, n, lag, rot, n_corr, n_tr, extra_tx, extra_rx in (
        ("sep_qpsk_0", 'qpsk', 1500, 0, 0, 1024, 0, 0, 0), ("sep_qpsk_p7", 'QPSK', 1500, 7, 1, 100, 0, 0, 0),
        ("sep_16_m5", '16qam', 1500, -5, 2, 1024, 0, 0, 0), ("sep_16_p10_tr", '16qam', 1500, 10, 3, 1024, 20, 0, 0),
        ("sep_64_m10_txlong", '64qam', 1500, -10, 1, 100, 0, 37, 0), ("sep_64_0", '64QAM', 600, 0, 3, 1024, 0, 0, 0),
        ("sep_256_p3_rxlong", '256qam', 1500, 3, 2, 1024, 0, 0, 41), ("sep_256_m1_tr", '256qam', 1501, -1, 0, 100, 5, 0, 0)):
    M = LEVELS[mod.lower()]
    def draw(count):
        return (2 * rng.integers(0, M, count) - (M - 1)) + 1j * (2 * rng.integers(0, M, count) - (M - 1))
    tx = draw(n + extra_tx)
    sigma = (1.0 / (M - 1)) / 2.17
    soft = tx[:n] / (M - 1) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    rx = delayed(soft, lag, draw(abs(lag)) / (M - 1)) * (1j) ** ((4 - rot) % 4)
    rx = np.concatenate((rx, draw(extra_rx) / (M - 1)))
    if n_tr:                                   # the transient goes in front of both streams
        tx, rx = np.concatenate((draw(n_tr), tx)), np.concatenate((draw(n_tr) / (M - 1), rx))
    _lines.lines.clear()
    nsymb, nerr, sep_hat = dc.qam_sep(tx.copy(), rx.copy(), mod, n_corr, n_tr)
    kmax, taumax = logged(r"\(1j\)\*\*(-?\d+), taumax = (-?\d+)")
    if (kmax, taumax) != (rot, lag):
        raise SystemExit("%s: the reference found (%d, %d), injected (%d, %d)" % (key, kmax, taumax, rot, lag))
    if not 0.01 <= nerr / nsymb <= 0.20:
        raise SystemExit("%s: %d errors in %d symbols is outside 1 %% ... 20 %%" % (key, nerr, nsymb))
    nmin = min(tx.size, rx.size) - n_tr
    K = 2 * (nmin // 2)
    lags = np.arange(K) - K // 2
    if unique_peak(exact_circular(quantise(rx[n_tr:n_tr + K], M), tx[n_tr:n_tr + K]), lags[np.abs(lags) <= n_corr]) != (rot, lag):
        raise SystemExit("%s: the exact search disagrees" % key)
    out[key + "_tx"], out[key + "_rx"] = np.stack((tx.real, tx.imag)).astype(np.int8), rx
    sep.append({"key": key, "mod": mod, "n_corr": n_corr, "n_transient": n_tr, "lag": lag, "rot": rot, "kmax": kmax, "taumax": taumax, "nsymb": int(nsymb),
                "nerr": int(nerr)})
out["sep"] = json.dumps(sep)

# ---------------------------------------------------------------------------------------------------------------- bpsk_bep, qpsk_bep
bp, qp = [], []
for key, n, lag, sign, soft, n_corr, n_tr in (("bpsk_hard_p4", 2000, 4, 0, False, 1024, 0), ("bpsk_hard_m6_inv", 2000, -6, 1, False, 64, 0),
                                              ("bpsk_soft_m3", 2000, -3, 0, True, 1024, 10), ("bpsk_soft_p9_inv", 1500, 9, 1, True, 256, 0)):
    tx = (2 * rng.integers(0, 2, n) - 1).astype(np.float64)
    sym = tx + ((1.3 if lag > 0 else 0.45) * rng.standard_normal(n) if soft else 0)   # (beyond +-3, int16((v + 1) / 2) is neither 0 nor 1)
    if not soft:
        flip = rng.random(n) < 0.05
        sym = np.where(flip, -sym, sym)
    rx = delayed(sym, lag, (2 * rng.integers(0, 2, abs(lag)) - 1).astype(np.float64)) * (-1) ** sign
    if n_tr:
        tx, rx = np.concatenate((rng.standard_normal(n_tr).round(), tx)), np.concatenate((rng.standard_normal(n_tr).round(), rx))
    _lines.lines.clear()
    count, errors = dc.bpsk_bep(tx.copy(), rx.copy(), n_corr, n_tr)
    kmax, taumax = logged(r"kmax =  (-?\d+), taumax = (-?\d+)")
    if (kmax, taumax) != (sign, lag):
        raise SystemExit("%s: the reference found (%d, %d), injected (%d, %d)" % (key, kmax, taumax, sign, lag))
    head = lambda v: np.concatenate((v[n_tr:n_tr + n_corr], np.zeros(max(0, n_corr - (v.size - n_tr)))))
    lags = np.arange(n_corr) - n_corr // 2
    if not soft and unique_peak(exact_circular(head(rx) + 0j, head(tx) + 0j), lags, True) != (sign, lag):
        raise SystemExit("%s: the exact search disagrees" % key)
    out[key + "_tx"], out[key + "_rx"] = tx, rx
    bp.append({"key": key, "n_corr": n_corr, "n_transient": n_tr, "soft": soft, "kmax": kmax, "taumax": taumax, "count": int(count), "errors": int(errors)})
out["bpsk"] = json.dumps(bp)

qpsk_error = None
for key, n, lag, rot, soft, n_corr, n_tr in (("qpsk_hard_p5_r1", 2000, 5, 1, False, 1024, 0), ("qpsk_hard_m8_r3", 2000, -8, 3, False, 64, 7),
                                             ("qpsk_soft_p2_r2", 1500, 2, 2, True, 256, 0), ("qpsk_soft_m4_r0", 1500, -4, 0, True, 1024, 0)):
    def draw(count):
        return (2 * rng.integers(0, 2, count) - 1) + 1j * (2 * rng.integers(0, 2, count) - 1)
    tx = draw(n)
    sym = tx + ((1.3 if lag > 0 else 0.45) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) if soft else 0)
    if not soft:
        sym = np.where(rng.random(n) < 0.05, -sym.real + 1j * sym.imag, sym)
    rx = delayed(sym, lag, draw(abs(lag))) * (1j) ** ((4 - rot) % 4)
    if n_tr:
        tx, rx = np.concatenate((draw(n_tr), tx)), np.concatenate((draw(n_tr), rx))
    try:
        dc.qpsk_bep(tx.copy(), rx.copy(), n_corr, n_tr)
        raise SystemExit("the reference's qpsk_bep returned: capture its results instead of the brute-force count")
    except TypeError as e:
        qpsk_error = "TypeError: " + str(e)
    head = lambda v: np.concatenate((v[n_tr:n_tr + n_corr], np.zeros(max(0, n_corr - (v.size - n_tr)))))
    lags = np.arange(n_corr) - n_corr // 2
    if not soft and unique_peak(exact_circular(head(rx), head(tx)), lags) != (rot, lag):
        raise SystemExit("%s: the exact search disagrees" % key)
    out[key + "_tx"], out[key + "_rx"] = tx, rx
    qp.append({"key": key, "n_corr": n_corr, "n_transient": n_tr, "lag": lag, "rot": rot, "soft": soft})
out["qpsk"] = json.dumps(qp)

np.savez_compressed(os.path.join(HERE, "g25_symerr.npz"), **out)

conventions = {
    "numpy": np.__version__,
    "signatures": {name: str(inspect.signature(getattr(dc, name))) for name in ("xcorr", "qam_sep", "qpsk_bep", "bpsk_bep")},
    "qpsk_bep_reference_raises": qpsk_error,
    "qpsk_bep_built": "the documented intent: taumax = int(lagmax[0]), as bpsk_bep computes it",
    "return_types": {"xcorr": "(complex128 ndarray, int64 ndarray)", "qam_sep": "(int, int, float)", "qpsk_bep": "(int, int64, int64, int64)",
                     "bpsk_bep": "(int, int64)"},
    "soft_counts": "qpsk_bep / bpsk_bep sum XORs of int16((v + 1) / 2), which are not 0 / 1 on soft values: the library returns the same integers",
    "search": {"qam_sep": "one lag-window correlation of quantised rx against tx over the whole stream, exact integers; candidates Re((1j)^k R0); ties to the "
                          "smallest k, then the first lag (the reference's pick on a tie depends on its FFT's rounding noise)",
               "qpsk_bep / bpsk_bep": "length-n_corr circular correlation of the two heads on the host: exact integers where both heads are integer-valued "
                                      "(and n_corr max|tx| max|rx| < 2^40), else the reference's float64 FFT expression; heads are taken as float64 / complex128"},
    "deliberate_differences": [
        "n_corr follows bit_errors' rules in all three counters: a positive even integer of at most 65536 (ValueError otherwise)",
        "ValueError for an unknown mod (as the reference), a non-finite sample, a stream of zero energy (the reference returns nan), a tx_data of qam_sep that "
        "is not integer-valued, an empty overlap in qam_sep (the reference divides by zero) and |(v + 1) / 2| >= 32768 in qpsk_bep / bpsk_bep",
        "xcorr: an x2 shorter than K raises ValueError (the reference fails to broadcast); the lag window is summed directly in float64",
        "qpsk_bep works (the reference raises TypeError with this NumPy)",
        "the log lines are the reference's; qam_sep's go through SEP_disp as there",
    ],
}
with open(os.path.join(HERE, "g25_conventions.json"), "w") as f:
    json.dump(conventions, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote g25_symerr.npz (%d arrays) and g25_conventions.json" % len(out))
