#!/usr/bin/env python3
"""G24: OFDM -- digitalcom.mux_pilot_blocks / ofdm_tx / chan_est_equalize / ofdm_rx (digitalcom.py:1284-1547) -- results from the REAL
reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_ofdm.py

  g24_ofdm.npz          "mux": JSON list of {key, N, nf, npb}: <key>_d (the data), <key>_y (the reference's mux_pilot_blocks).
                        "cases": JSON list of {key, symbols, nf, nc, npb, cp, ncp, rx}: <key>_data (symbols nf + 3 QAM values: the tail is what
                        ofdm_tx truncates), <key>_tx = ofdm_tx(data, nf, nc, npb, cp, ncp), and per receiver mode in rx, {mode, npb, ht}:
                        <key>_<mode>_z, <key>_<mode>_H = ofdm_rx(rxin, nf, nc, npb, cp, ncp, alpha, hc if ht else None) with rxin =
                        scipy.signal.lfilter(hc, 1, <key>_tx) (not stored: a test forms it the same way) and the ofdm_rx docstring's hc.
                        Modes: "none" (npb = 0), "ideal" (npb = -1, ht), "pilot" (npb > 0, ht: pilots removed, data divided by the channel of
                        ht, H the last recursive estimate).
                        "hc", "alpha".
  g24_conventions.json  signatures, what the reference does where the library deliberately differs, the deliberate differences
"""
import contextlib
import inspect
import io
import json
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402
from scipy import signal  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402

rng = np.random.default_rng(2424)
out = {}
HC = np.array([1.0, 0.1, -0.05, 0.15, 0.2, 0.05])
ALPHA = 0.9
# (symbols, nf, nc, npb, cp, ncp)
SHAPES = [(100, 32, 64, 10, True, 8), (99, 32, 64, 10, True, 8), (7, 2, 64, 2, True, 64), (8, 62, 64, 3, True, 1), (5, 30, 128, 0, False, 7),
          (9, 100, 256, 4, True, 0), (0, 32, 64, 0, True, 8), (12, 48, 96, 5, True, 12), (2, 510, 1024, 0, True, 16), (1, 4094, 4096, 0, True, 3)]


def quiet(fn):
    """the reference prints a shape and plots its estimates: neither belongs to the result"""
    import matplotlib.pyplot as plt
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return fn()
        finally:
            plt.close("all")


def outcome(fn):
    try:
        quiet(fn)
        return "returns"
    except Exception as e:  # noqa: BLE001
        return type(e).__name__


def qam16(n):
    return (rng.integers(0, 4, n) * 2 - 3) + 1j * (rng.integers(0, 4, n) * 2 - 3)


mux = []
for N in (0, 1, 2, 3, 4, 8, 9, 18, 19):
    for npb in (2, 3, 4, 10):
        nf = 2 if (N + npb) % 2 else 6
        key = "mux_%d_%d" % (N, npb)
        d = qam16(N * nf).reshape(N, nf)
        out[key + "_d"], out[key + "_y"] = d, dc.mux_pilot_blocks(d, npb)
        mux.append({"key": key, "N": N, "nf": nf, "npb": npb})
out["mux"] = json.dumps(mux)

cases = []
for i, (symbols, nf, nc, npb, cp, ncp) in enumerate(SHAPES):
    key = "c%d" % i
    data = qam16(symbols * nf + 3)
    tx = quiet(lambda: dc.ofdm_tx(data, nf, nc, npb, cp, ncp))
    assert tx.dtype == np.complex128
    rxin = signal.lfilter(HC, 1, tx) if tx.size else tx
    modes = []
    for mode, rnpb, ht in (("none", 0, False), ("ideal", -1, True), ("pilot", npb if npb > 0 else 3, True)):
        if mode == "pilot" and rxin.size // (nc + ncp) == 0:
            continue    # no symbol, no pilot: the reference's H is unbound
        z, H = quiet(lambda: dc.ofdm_rx(rxin, nf, nc, rnpb, cp, ncp, alpha=ALPHA, ht=HC if ht else None))
        out["%s_%s_z" % (key, mode)], out["%s_%s_H" % (key, mode)] = z, np.asarray(H)
        modes.append({"mode": mode, "npb": rnpb, "ht": ht})
    out[key + "_data"], out[key + "_tx"] = data, tx
    cases.append({"key": key, "symbols": symbols, "nf": nf, "nc": nc, "npb": npb, "cp": cp, "ncp": ncp, "rx": modes})
out["cases"] = json.dumps(cases)
out["hc"], out["alpha"] = HC, np.float64(ALPHA)
np.savez_compressed(os.path.join(HERE, "g24_ofdm.npz"), **out)

x64 = quiet(lambda: dc.ofdm_tx(qam16(64), 32, 64, 0, True, 8))
conv = {
    "signatures": {n: str(inspect.signature(getattr(dc, n))) for n in ("mux_pilot_blocks", "ofdm_tx", "chan_est_equalize", "ofdm_rx")},
    "reference_behaviour": {
        "ofdm_tx(complex64) dtype": str(quiet(lambda: dc.ofdm_tx(qam16(64).astype(np.complex64), 32, 64)).dtype),
        "ofdm_rx(npb > 0, ht=None)": outcome(lambda: dc.ofdm_rx(x64, 32, 64, 2, True, 8)),
        "ofdm_rx(npb = -1, ht=None)": outcome(lambda: dc.ofdm_rx(x64, 32, 64, -1, True, 8)),
        "ofdm_tx(npb = 1)": outcome(lambda: dc.ofdm_tx(qam16(64), 32, 64, 1)),
        "ofdm_tx(odd nf)": outcome(lambda: dc.ofdm_tx(qam16(62), 31, 64)),
        "ofdm_tx(nf = nc)": outcome(lambda: dc.ofdm_tx(qam16(64), 64, 64)),
        "ofdm_rx(empty x, npb = 0)": outcome(lambda: dc.ofdm_rx(np.zeros(0, dtype=complex), 32, 64, 0, True, 8)),
        "ofdm_rx(empty x, npb > 0, ht)": outcome(lambda: dc.ofdm_rx(np.zeros(0, dtype=complex), 32, 64, 2, True, 8, ht=HC)),
    },
    "deliberate_differences": {
        "no_print_no_plots": "ofdm_tx prints no shape and chan_est_equalize / ofdm_rx plot nothing.",
        "dtype": "complex64 / float32 input gives complex64 output, computed in float64 and rounded once; everything else gives complex128 (the reference always returns complex128).  H is float64 ones for npb = 0 and complex128 otherwise, as in the reference.",
        "estimator_intent": "npb > 0 with ht=None divides each data symbol by the running estimate of the latest pilot at or before it (the reference's documented intent; its isinstance test makes that branch dead code and the call raises).  With ht given the data symbols are divided by the channel of ht and H is the last recursive estimate, as the reference computes.",
        "value_errors": "ValueError for an odd nf, nf < 2 or nf > nc - 2; npb = 1; npb < 0 (tx), npb < -1 (rx); ncp < 0 or ncp > nc; npb = -1 without ht; len(ht) > nc or an empty ht.",
        "empty_input": "an empty input, or one shorter than a symbol, gives empty arrays: H = ones(nf) for npb = 0, the channel of ht for npb = -1, all nan for npb > 0 (no pilot was seen; the reference's H is unbound there).  ofdm_tx with npb > 0 and no data symbol gives the reference's one all-zero symbol.",
        "rows": "ofdm_tx_rows / ofdm_rx_rows take a frame set, one frame per row, and equal the 1-D call on each row; ofdm_rx_rows returns (z2d, H2d).",
        "host_route": "an nc that is not a power of two in 64 ... 4096 runs the float64 NumPy restatement (ofdm_tx_host / ofdm_rx_host), logged at INFO.",
    },
}
with open(os.path.join(HERE, "g24_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("g24: %d mux shapes, %d cases, %d bytes" % (len(mux), len(cases), os.path.getsize(os.path.join(HERE, "g24_ofdm.npz"))))
