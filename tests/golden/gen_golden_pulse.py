#!/usr/bin/env python3
"""G26: pulse shaping and matched filtering -- qam_gray_encode_bb (digitalcom.py:1626-1681), mpsk_gray_encode_bb (:1784-1826), sigsys.nrz_bits2
(sigsys.py:2163-2211) and signal.lfilter(b, 1, x)[start::ns] on noisy waveforms -- results from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_pulse.py

  g26_pulse.npz         "enc": JSON list of {key, kind, mod, ns, pulse, alpha, m_span, n_symb}: <key>_bits (uint8, the ext_data) -> <key>_x (what the
                        transmitter returns: float64 for mod 2, else complex128) and <key>_b (its b; the scalar 1 for ns == 1).
                        "mf": JSON list of {key, enc, ns, pulse, m_span, starts}: <key>_x (the transmitter's waveform of case `enc` plus noise, complex128 or
                        float64), <key>_b (the matched filter: the transmitter's b) -> <key>_z<start> = signal.lfilter(b, 1, x)[start::ns].
                        "nrz": JSON list of {key, ns, pulse, alpha, m}: <key>_data (uint8) -> <key>_x, <key>_b of nrz_bits2.
  g26_conventions.json  signatures, the NumPy / SciPy versions, and the observation that a complex array divided by a real scalar is multiplied by the
                        scalar's reciprocal component by component (the x / x_m of qam_gray_encode_bb)
"""
import inspect
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("SK_DSP_COMM_SRC", "/root/reference/src"))

import numpy as np  # noqa: E402
import scipy  # noqa: E402
from scipy import signal  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402
from sk_dsp_comm import sigsys as ss  # noqa: E402

rng = np.random.default_rng(2626)
out = {}
NS = (1, 2, 3, 8, 16)
PULSES = ('rect', 'rc', 'src')
ORDERS = [('qam', m) for m in (2, 4, 16, 256)] + [('mpsk', m) for m in (2, 8, 32)]
ENCODERS = {'qam': dc.qam_gray_encode_bb, 'mpsk': dc.mpsk_gray_encode_bb}

# ---- the transmitters: every order at every ns; pulse and span rotate so that every (ns, pulse) pair and both spans of rc / src occur
enc = []
for i, (kind, mod) in enumerate(ORDERS):
    for j, ns in enumerate(NS):
        pulse, m_span, alpha = PULSES[(i + j) % 3], (2, 6)[(i + j // 3) % 2], (0.35, 0.25, 0.5)[(i + 2 * j) % 3]
        n_symb = 300 if (i, j) == (2, 3) else (61, 40, 53)[(i + j) % 3]
        bps = int(np.log2(mod))
        bits = rng.integers(0, 2, n_symb * bps).astype(np.uint8)
        x, b, data = ENCODERS[kind](None, ns, mod, pulse, alpha, m_span, ext_data=bits.astype(np.int64))   # (uint8 bits would wrap in 2 * data - 1)
        assert np.array_equal(data, bits) and len(x) == n_symb * ns
        key = "e%02d" % len(enc)
        enc.append(dict(key=key, kind=kind, mod=mod, ns=ns, pulse=pulse, alpha=alpha, m_span=m_span, n_symb=n_symb))
        out[key + "_bits"], out[key + "_x"], out[key + "_b"] = bits, np.asarray(x), np.asarray(b, dtype=np.float64)
pairs = {(c["ns"], c["pulse"]) for c in enc}
assert pairs == {(ns, p) for ns in NS for p in PULSES}, sorted(pairs)
assert {(c["pulse"], c["m_span"]) for c in enc} >= {(p, m) for p in ('rc', 'src') for m in (2, 6)}
out["enc"] = json.dumps(enc)

# ---- the matched filter behind a noisy channel: lfilter at the full rate, read at the symbol rate
mf = []
for c in enc:
    if c["ns"] == 1 or len(mf) >= 9 or (c["ns"], c["pulse"]) in {(m_["ns"], m_["pulse"]) for m_ in mf}:
        continue
    x, b = out[c["key"] + "_x"], out[c["key"] + "_b"]
    noise = 0.1 * (rng.standard_normal(x.size) + (1j * rng.standard_normal(x.size) if np.iscomplexobj(x) else 0))
    xn = x + noise
    key = "m%02d" % len(mf)
    starts = sorted({0, 5, 2 * c["m_span"] * c["ns"]})
    mf.append(dict(key=key, enc=c["key"], ns=c["ns"], pulse=c["pulse"], m_span=c["m_span"], starts=starts))
    out[key + "_x"], out[key + "_b"] = xn, b
    for start in starts:
        out[key + "_z%d" % start] = signal.lfilter(b, 1, xn)[start::c["ns"]]
assert {np.asarray(out[m_["key"] + "_x"]).dtype.kind for m_ in mf} == {"f", "c"}
out["mf"] = json.dumps(mf)

# ---- nrz_bits2
nrz = []
for ns, pulse, alpha, m in ((8, 'rect', 0.25, 6), (3, 'rc', 0.25, 2), (16, 'src', 0.35, 6), (2, 'src', 0.5, 2), (1, 'rect', 0.25, 6)):
    data = rng.integers(0, 2, 47).astype(np.uint8)
    x, b = ss.nrz_bits2(data.astype(np.int64), ns, pulse, alpha, m)
    key = "n%02d" % len(nrz)
    nrz.append(dict(key=key, ns=ns, pulse=pulse, alpha=alpha, m=m))
    out[key + "_data"], out[key + "_x"], out[key + "_b"] = data, np.asarray(x), np.asarray(b, dtype=np.float64)
out["nrz"] = json.dumps(nrz)

# ---- complex array / real scalar
obs = {}
z = rng.standard_normal(4000) + 1j * rng.standard_normal(4000)
for x_m in (3.0, 7.0, 15.0):
    q = z / x_m
    as_product = bool(np.array_equal(q.real, z.real * (1 / x_m)) and np.array_equal(q.imag, z.imag * (1 / x_m)))
    as_quotient = bool(np.array_equal(q.real, z.real / x_m) and np.array_equal(q.imag, z.imag / x_m))
    obs["x_m=%d" % x_m] = dict(equals_component_times_reciprocal=as_product, equals_component_quotient=as_quotient)

np.savez_compressed(os.path.join(HERE, "g26_pulse.npz"), **out)
conv = {
    "numpy": np.__version__,
    "scipy": scipy.__version__,
    "signatures": {f.__name__: str(inspect.signature(f)) for f in (dc.qam_gray_encode_bb, dc.mpsk_gray_encode_bb, ss.nrz_bits2)},
    "complex_array_divided_by_real_scalar": obs,
    "notes": [
        "qam_gray_encode_bb returns x / x_m behind the shaping filter: NumPy evaluates a complex array divided by a real scalar as re * (1 / x_m), im * (1 / x_m)",
        "lfilter with a = 1 runs np.convolve: its summation order is the dot product's, not lfilter's documented one; the fixtures are met within the order bound",
        "mod 2 transmitters return a real waveform; the _rows forms return it as a complex array with imaginary part 0",
    ],
}
with open(os.path.join(HERE, "g26_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("g26: %d transmitter cases, %d matched-filter cases, %d nrz cases, %d bytes" % (len(enc), len(mf), len(nrz), os.path.getsize(os.path.join(HERE, "g26_pulse.npz"))))
print(json.dumps(obs))
