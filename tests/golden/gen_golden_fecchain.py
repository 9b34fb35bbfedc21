#!/usr/bin/env python3
"""G21: the FEC chain around the Viterbi decoder -- fec_conv.FECConv.conv_encoder / puncture / depuncture (fec_conv.py:501-712) and
digitalcom.bit_errors (digitalcom.py:353-415) -- results, warnings, return types and failures from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_fecchain.py

  g21_fecchain.npz      "enc": JSON list of conv_encoder cases {key, G, n, state, state_out, out_dtype, out_type}: <key>_in / <key>_out, uint8
                        "punct": JSON list of puncture / depuncture cases {key, fn, pattern, n, erase_value, warnings, out_dtype}: <key>_in /
                        <key>_out (puncture: uint8 bits; depuncture: float64 on a grid of 1/8)
                        "ber": JSON list of bit_errors cases {key, n_corr, n_transient, same, count, errors, kmax, taumax}: <key>_tx / <key>_rx, uint8
  g21_conventions.json  signatures, return types, how the reference fails on patterns the kernels refuse, the deliberate differences

Every bit_errors case is written only if, in exact integer arithmetic, its correlation maximum is attained ONCE and the two phases' maxima
differ: no fixture depends on the rounding noise of the reference's FFT (the generator refuses the case otherwise).
"""
import inspect
import json
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402
from sk_dsp_comm import fec_conv as fc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(2121)

CODES = [('111', '101'), ('11101', '10011'), ('1111001', '1011011'), ('111101011', '101110001'),
         ('111', '111', '101'), ('111101', '101011', '100111'), ('11110111', '11011001', '10010101'),
         ('0111', '0101'), ('0111', '1101', '1011')]          # the last two: polynomials that start with 0 (rate 1/2 feeds the input in anyway)
out = {}


def with_warnings(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = fn()
    return r, [str(v.message) for v in w]


def outcome(fn):
    try:
        (y, w) = with_warnings(fn)
        y = np.asarray(y)
        return {"shape": list(y.shape), "dtype": str(y.dtype), "warnings": w}
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__, "message": str(e)}


# ---- conv_encoder ------------------------------------------------------------------------------------------------------------
enc = []
for G in CODES:
    K = len(G[0])
    cc = fc.FECConv(G, 10)
    for n in sorted({1, K - 2, K - 1, K, 17, 200}):
        for sname, state in (("zero", '0' * (K - 1)), ("one", '1' * (K - 1)), ("rand", "".join(str(v) for v in rng.integers(0, 2, K - 1)))):
            bits = rng.integers(0, 2, n)
            y, s = cc.conv_encoder(bits, state)
            assert np.all((np.asarray(y) == 0) | (np.asarray(y) == 1)) and len(y) == len(G) * n and len(s) == K - 1
            key = "enc_%d_%s_%d_%s" % (len(G), G[0], n, sname)
            out[key + "_in"], out[key + "_out"] = bits.astype(np.uint8), np.asarray(y).astype(np.uint8)
            enc.append({"key": key, "G": list(G), "n": n, "state": state, "state_out": s, "out_dtype": str(np.asarray(y).dtype), "out_type": type(y).__name__})
out["enc"] = np.array(json.dumps(enc))

# ---- puncture / depuncture ---------------------------------------------------------------------------------------------------
punct = []
cc = fc.FECConv(('111', '101'), 10)
PATTERNS = [('110', '101'), ('1101', '1011'), ('1000101', '1111010'), ('1', '1'), ('1001011', '1110100')]   # the third keeps 3 and 5 bits: the reference fails on it
for pat in PATTERNS:
    L_pp, L1 = len(pat[0]), pat[0].count('1')
    # zero periods, exactly one, odd (one warning pair), a non-multiple (the other), both, and >= 40 periods
    for fn, per in (("puncture", 2 * L_pp), ("depuncture", 2 * L1)):
        lens = [per - 2 if per > 2 else 0, per, per + 1, 3 * per + 2 if per > 2 else 6, 3 * per + 3 if per > 2 else 7, 41 * per]
        for n in sorted(set(lens)):
            for erase in ((None,) if fn == "puncture" else (3.5, -2.25)):
                if n == 0:
                    continue          # (the reference reshapes an empty array with a zero period count: recorded under conventions)
                v = rng.integers(0, 2, n).astype(np.float64) if fn == "puncture" else np.round(rng.uniform(-1, 8, n) * 8) / 8
                if fn == "puncture":
                    r = outcome(lambda: cc.puncture(v, pat))
                    y, w = with_warnings(lambda: cc.puncture(v, pat)) if "raises" not in r else (None, None)
                else:
                    r = outcome(lambda: cc.depuncture(v, pat, erase))
                    y, w = with_warnings(lambda: cc.depuncture(v, pat, erase)) if "raises" not in r else (None, None)
                key = "%s_%s_%d%s" % (fn[:3], pat[0], n, "" if erase in (None, 3.5) else "_e")
                if y is None:
                    punct.append({"key": key, "fn": fn, "pattern": list(pat), "n": n, "erase_value": erase, "raises": r["raises"], "message": r["message"]})
                    continue
                y = np.asarray(y)
                out[key + "_in"] = v.astype(np.uint8) if fn == "puncture" else v
                out[key + "_out"] = y.astype(np.uint8) if fn == "puncture" else y.astype(np.float64)
                assert np.array_equal(out[key + "_out"], y)
                punct.append({"key": key, "fn": fn, "pattern": list(pat), "n": n, "erase_value": erase, "warnings": w, "out_dtype": str(y.dtype)})
out["punct"] = np.array(json.dumps(punct))


# ---- bit_errors --------------------------------------------------------------------------------------------------------------
def exact_search(tx, rx, n_corr):
    """the circular correlation by direct integer products: (unique maximum?, phase maxima differ?, kmax, taumax)"""
    a, b = np.zeros(n_corr, dtype=np.int64), np.zeros(n_corr, dtype=np.int64)
    t, r = tx[:n_corr].astype(np.int64), rx[:n_corr].astype(np.int64)
    a[:t.size], b[:r.size] = 2 * t - 1, 2 * r - 1
    idx = (np.arange(n_corr)[:, None] + np.arange(n_corr)[None, :]) % n_corr      # R0[k] = sum_m b[m + k] a[m]
    R0 = np.fft.fftshift((b[idx] * a[None, :]).sum(axis=1))
    R1 = -R0
    kmax = 1 if R1.max() > R0.max() else 0
    R = R1 if kmax else R0
    return int(np.sum(R == R.max())) == 1, R0.max() != R1.max(), kmax, int(np.argmax(R)) - n_corr // 2


ber = []


def ber_case(key, tx, rx, n_corr, n_transient, same=False):
    unique, differ, kmax, taumax = exact_search(tx[n_transient:], rx[n_transient:], n_corr)
    assert unique and differ, "%s: the exact correlation maximum is not unique -- the reference's pick would depend on rounding noise; case refused" % key
    t = tx.astype(np.float64)
    count, errors = dc.bit_errors(t, t if same else rx.astype(np.float64), n_corr, n_transient)      # same: tx is rx, one object
    out[key + "_tx"], out[key + "_rx"] = tx.astype(np.uint8), rx.astype(np.uint8)
    ber.append({"key": key, "n_corr": n_corr, "n_transient": n_transient, "same": same, "count": int(count), "errors": int(errors), "kmax": kmax,
                "taumax": taumax, "types": [type(count).__name__, type(errors).__name__]})


def channel(tx, delay, invert, p_err, n_rx=None):
    """rx = tx delayed by `delay` (negative: advanced), inverted, with a fraction p_err of its bits flipped"""
    n_rx = len(tx) if n_rx is None else n_rx
    rx = rng.integers(0, 2, n_rx)
    if delay >= 0:
        m = min(n_rx - delay, len(tx))
        rx[delay:delay + m] = tx[:m]
    else:
        m = min(n_rx, len(tx) + delay)
        rx[:m] = tx[-delay:-delay + m]
    rx = rx ^ (rng.random(n_rx) < p_err)
    return (1 - rx) if invert else rx


grid = [(64, 0, 700, 0, 0, 0.05), (64, 7, 900, 5, 1, 0.05), (64, 0, 2000, -9, 0, 0.0), (64, 7, 700, 20, 0, 0.05), (64, 0, 1500, -20, 1, 0.05),
        (256, 0, 700, 3, 1, 0.05), (256, 7, 5000, -20, 0, 0.05), (256, 0, 20000, 20, 1, 0.0), (256, 7, 3000, 0, 1, 0.05), (256, 0, 999, -1, 0, 0.05),
        (1024, 0, 700, 4, 0, 0.05), (1024, 7, 800, -6, 1, 0.05), (1024, 0, 1024, 11, 0, 0.05), (1024, 7, 20000, -20, 1, 0.05), (1024, 0, 20000, 20, 0, 0.05),
        (1024, 0, 5000, 0, 0, 0.0), (1024, 7, 5000, 1, 1, 0.0), (1024, 0, 3001, -13, 0, 0.05), (1024, 7, 10007, 17, 1, 0.05), (1024, 0, 1031, 2, 1, 0.05),
        (64, 0, 20000, 10, 0, 0.05), (256, 0, 701, -7, 1, 0.05), (1024, 0, 900, -3, 1, 0.0), (256, 7, 1500, 15, 0, 0.05), (1024, 7, 2048, -2, 0, 0.05),
        (64, 7, 4097, 1, 1, 0.05)]
for i, (n_corr, n_tr, n, delay, inv, p) in enumerate(grid):
    tx = rng.integers(0, 2, n)
    ber_case("ber_%02d" % i, tx, channel(tx, delay, inv, p), n_corr, n_tr)
tx = rng.integers(0, 2, 3000)
ber_case("ber_rx_longer", tx, channel(tx, 6, 0, 0.05, 3500), 1024, 0)
ber_case("ber_rx_shorter", tx, channel(tx, -4, 1, 0.05, 2200), 1024, 0)
ber_case("ber_rx_longer_adv", tx, channel(tx, -5, 0, 0.05, 3400), 256, 7)
ber_case("ber_same", tx, tx, 1024, 0, same=True)
out["ber"] = np.array(json.dumps(ber))
np.savez_compressed(os.path.join(HERE, "g21_fecchain.npz"), **out)

# ---- conventions -------------------------------------------------------------------------------------------------------------
v60 = rng.integers(0, 2, 60).astype(np.float64)
b = rng.integers(0, 2, 2000)
count, errors = dc.bit_errors(b.astype(np.float64), b.astype(np.float64))
bad = b.astype(np.float64).copy()
bad[5] = 2.0
conv = {
    "signatures": {
        "conv_encoder": [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(fc.FECConv.conv_encoder).parameters.values()],
        "puncture": [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(fc.FECConv.puncture).parameters.values()],
        "depuncture": [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(fc.FECConv.depuncture).parameters.values()],
        "bit_errors": [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(dc.bit_errors).parameters.values()],
    },
    "return_types": {
        "conv_encoder": [type(v).__name__ for v in fc.FECConv(('111', '101'), 10).conv_encoder(np.array([1, 0, 1]), '00')],
        "conv_encoder_out_dtype": str(np.asarray(fc.FECConv(('111', '101'), 10).conv_encoder(np.array([1, 0, 1]), '00')[0]).dtype),
        "puncture": outcome(lambda: cc.puncture(v60)),
        "depuncture": outcome(lambda: cc.depuncture(v60[:40])),
        "bit_errors": [type(count).__name__, type(errors).__name__],
    },
    "unequal_patterns": {
        "puncture_unequal_length": outcome(lambda: cc.puncture(v60, ('110', '1011'))),
        "puncture_unequal_ones": outcome(lambda: cc.puncture(v60, ('110', '100'))),
        "depuncture_unequal_length": outcome(lambda: cc.depuncture(v60[:40], ('110', '1011'))),
        "depuncture_unequal_ones": outcome(lambda: cc.depuncture(v60[:40], ('110', '100'))),
        "puncture_empty": outcome(lambda: cc.puncture(np.zeros(0))),
        "depuncture_empty": outcome(lambda: cc.depuncture(np.zeros(0))),
    },
    "bit_errors": {
        "odd_n_corr": outcome(lambda: dc.bit_errors(b.astype(np.float64), b.astype(np.float64), 255)),
        "value_2": outcome(lambda: dc.bit_errors(bad, b.astype(np.float64))),
        "integer_input": outcome(lambda: dc.bit_errors(b, b)),
        "empty_after_transient": outcome(lambda: dc.bit_errors(b[:5].astype(np.float64), b[:5].astype(np.float64), 64, 5)),
    },
    "deliberate_differences": {
        "bit_values": "bit_errors: values other than 0 / 1 raise ValueError; the reference correlates and counts whatever 2 x - 1 and int16((x + 1) / 2) make of them",
        "odd_n_corr": "bit_errors: an odd n_corr gives the reference's warning, then ValueError; the reference goes on with lag 0 at a half-integer index",
        "n_corr_max": "bit_errors: n_corr > 65536 raises ValueError (the exactness argument of the integer search is made for these sizes)",
        "ties": "bit_errors: where the exact correlation maximum is attained more than once (or both phases share it) the reference's pick is decided by "
                "its FFT's rounding noise; this picks phase 0 unless phase 1's maximum is strictly larger, and the first index attaining the maximum",
        "empty": "bit_errors: streams with no bits behind the transient raise ValueError",
        "patterns": "puncture_rows / depuncture_rows: patterns of more than 64 digits, of unequal length, or with unequal numbers of ones raise ValueError "
                    "(unequal_patterns and the ('1000101', '1111010') cases record what the reference does with the last two: its puncture raises from "
                    "take / reshape / hstack as soon as there is one period, its depuncture sizes everything by the FIRST pattern's ones and returns a "
                    "result whose G2 column is not the inverse of any puncturing); the 1-D host methods are unchanged and make no claim for such patterns",
        "rows": "conv_encoder_rows, puncture_rows, depuncture_rows and bit_errors_rows are beyond the reference; each row equals the 1-D result",
    },
}
with open(os.path.join(HERE, "g21_conventions.json"), "w") as fh:
    json.dump(conv, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("g21: %d encoder, %d puncture / depuncture, %d bit_errors cases, %d bytes" % (len(enc), len(punct), len(ber), os.path.getsize(os.path.join(HERE, "g21_fecchain.npz"))))
