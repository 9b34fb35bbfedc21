#!/usr/bin/env python3
"""G23: the AWGN channel and the bit sources -- sigsys.cpx_awgn / cpx_awgn2 (sigsys.py:2335-2454), digitalcom.awgn_channel
(digitalcom.py:1259-1281), sigsys.m_seq / pn_gen (sigsys.py:1947-2050) -- results from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_channel.py

  g23_channel.npz       "mseq": m = 2 ... 16, mseq_<m> = np.packbits of the reference's period; "pn": JSON list of {key, n_bits, m}, <key> =
                        np.packbits of the reference's pn_gen; "errors": what m = 1 and m = 17 raise.
                        "awgn": JSON list of {key, fn, es_n0, ns, var_w, seed, in_dtype, ref_in, tag}: <key>_x, <key>_y.  The reference's own
                        function ran with numpy.random.randn replaced, for the call, by this library's host normals of `seed`
                        (_ffi.normals_host: row 0 from index 0; the complex stream's real parts on the first call, its imaginary parts on
                        the second), so everything but the draw is the reference's arithmetic.  ref_in "widened": it ran on
                        <key>_x.astype(complex128) (the exact widening of a complex64 input: the library forms the sum in float64 too).
                        "chan": JSON list of {key, eb_n0_dB, seed, n, margin}: <key>_x (uint8), <key>_y (float64) of awgn_channel with the
                        REAL stream of `seed`; margin = min |2 b - 1 + sigma z|.
  g23_conventions.json  signatures, how the reference treats an empty input, the deliberate differences

The generator REFUSES to write an awgn_channel case with a margin below 1e-9: no fixture depends on which way a rounding error tips a
decision.  No element is excluded from any comparison.
"""
import inspect
import json
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, os.path.join(HERE, "..", "..", "scikit-dsp-comm_amd"))

import numpy as np  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402
from sk_dsp_comm import sigsys as ss  # noqa: E402
from sk_dsp_comm_amd import _ffi  # noqa: E402  (the host restatement of the draw only: no GPU, no library)

rng = np.random.default_rng(2323)
out = {}


class HostDraw:
    """numpy.random.randn for one call of the reference: the library's host normals of a seed"""

    def __init__(self, seed, cpx):
        self.seed, self.cpx, self.calls = seed, cpx, 0

    def __call__(self, n):
        z = _ffi.normals_host(self.seed, 0, 0, n, self.cpx)
        part = (z.real, z.imag)[self.calls] if self.cpx else z
        self.calls += 1
        return np.array(part)


def with_draw(draw, fn):
    keep = np.random.randn
    np.random.randn = draw
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn()
    finally:
        np.random.randn = keep


def outcome(fn):
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            y = np.asarray(fn())
        return {"shape": list(y.shape), "dtype": str(y.dtype), "warnings": [str(v.message) for v in w]}
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__, "message": str(e)}


# ---------------------------------------------------------------------------------------------- m_seq, pn_gen
for m in range(2, 17):
    c = ss.m_seq(m)
    assert c.dtype == np.float64 and c.size == 2 ** m - 1 and set(np.unique(c)) <= {0.0, 1.0}
    out["mseq_%d" % m] = np.packbits(c.astype(np.uint8))
pn = []
for n_bits, m in ((50, 4), (1000, 5), (1, 2), (31, 5), (32, 5), (70000, 16)):
    y = ss.pn_gen(n_bits, m)
    assert y.dtype == np.float64 and y.shape == (n_bits,)
    key = "pn_%d_%d" % (n_bits, m)
    out[key] = np.packbits(y.astype(np.uint8))
    pn.append({"key": key, "n_bits": n_bits, "m": m})
errors = {str(m): outcome(lambda m=m: ss.m_seq(m)) for m in (1, 17)}

# ---------------------------------------------------------------------------------------------- cpx_awgn, cpx_awgn2
awgn = []


def signal(n, cpx, dc_offset):
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cpx else 0.0)
    if dc_offset:
        x = x + 10.0 * np.std(x) * ((1 + 0.5j) if cpx else 1.0) if n > 1 else x + 10.0
    return x if cpx else x.real


def add_awgn(fn, n, cpx, es_n0, ns, var_w=0.0, c64=False, dc_offset=False):
    seed = int(rng.integers(0, 2 ** 63))
    x = signal(n, cpx, dc_offset)
    if c64:
        x = x.astype(np.complex64 if cpx else np.float32)
    ref_x = x.astype(np.complex128 if cpx else np.float64)       # (exact)
    args = (ref_x, es_n0, ns) if fn == "cpx_awgn" else (ref_x, es_n0, ns, var_w)
    y = with_draw(HostDraw(seed, True), lambda: getattr(ss, fn)(*args))
    assert y.dtype == np.complex128 and y.shape == (n,)
    key = "awgn_%d" % len(awgn)
    out[key + "_x"], out[key + "_y"] = x, y
    awgn.append({"key": key, "fn": fn, "es_n0": es_n0, "ns": ns, "var_w": var_w, "seed": seed, "in_dtype": str(x.dtype),
                 "ref_in": "widened" if c64 else "same", "tag": "dc" if dc_offset else ""})


for n in (1, 2, 17):
    for cpx in (False, True):
        add_awgn("cpx_awgn", n, cpx, 10, 1)
        add_awgn("cpx_awgn2", n, cpx, 10, 8, -40.0)
add_awgn("cpx_awgn", 2049, True, 0, 1)
add_awgn("cpx_awgn", 2049, False, 40, 8)
add_awgn("cpx_awgn", 2049, True, 10, 8, dc_offset=True)
add_awgn("cpx_awgn", 2049, True, 10, 1, c64=True)
add_awgn("cpx_awgn", 17, False, 0, 8, c64=True)
add_awgn("cpx_awgn2", 2049, True, 40, 8, -40.0)
add_awgn("cpx_awgn2", 2049, False, 0, 1, 0.0)
add_awgn("cpx_awgn2", 17, True, 10, 1, 0.0, dc_offset=True)
add_awgn("cpx_awgn2", 17, True, 40, 8, -40.0, c64=True)
add_awgn("cpx_awgn2", 17, False, 10, 1, 0.0, dc_offset=True)

# ---------------------------------------------------------------------------------------------- awgn_channel
chan = []
for n, eb in ((1, 4.0), (2, 0.0), (17, 10.0), (2049, 4.0), (2049, -3.0)):
    seed = int(rng.integers(0, 2 ** 63))
    x = rng.integers(0, 2, n)
    y = with_draw(HostDraw(seed, False), lambda: dc.awgn_channel(x, eb))
    v = (2 * x - 1) + np.sqrt(10 ** (-eb / 10) / 2) * _ffi.normals_host(seed, 0, 0, n, False)
    margin = float(np.min(np.abs(v)))
    if margin < 1e-9:
        raise SystemExit("awgn_channel case (n = %d, eb = %g): margin %.3g below 1e-9 -- choose another seed, exclude nothing" % (n, eb, margin))
    assert y.dtype == np.float64 and set(np.unique(y)) <= {0.0, 1.0}
    key = "chan_%d" % len(chan)
    out[key + "_x"], out[key + "_y"] = x.astype(np.uint8), y
    chan.append({"key": key, "eb_n0_dB": eb, "seed": seed, "n": n, "margin": margin})

out["mseq"] = np.array(json.dumps(list(range(2, 17))))
out["pn"] = np.array(json.dumps(pn))
out["errors"] = np.array(json.dumps(errors))
out["awgn"] = np.array(json.dumps(awgn))
out["chan"] = np.array(json.dumps(chan))
np.savez_compressed(os.path.join(HERE, "g23_channel.npz"), **out)

conventions = {
    "signatures": {name: str(inspect.signature(getattr(mod, name))) for mod, name in
                   ((ss, "cpx_awgn"), (ss, "cpx_awgn2"), (ss, "m_seq"), (ss, "pn_gen"), (dc, "awgn_channel"))},
    "reference_empty_input": {
        "cpx_awgn": outcome(lambda: ss.cpx_awgn(np.zeros(0), 10, 1)),
        "cpx_awgn2": outcome(lambda: ss.cpx_awgn2(np.zeros(0), 10, 1)),
        "awgn_channel": outcome(lambda: dc.awgn_channel(np.zeros(0, dtype=int), 10)),
        "pn_gen": outcome(lambda: ss.pn_gen(0, 5)),
    },
    "reference_result_dtype": {"cpx_awgn(float32)": str(with_draw(HostDraw(1, True), lambda: ss.cpx_awgn(np.ones(4, np.float32), 10, 1)).dtype),
                               "m_seq": "float64", "pn_gen": "float64", "awgn_channel": "float64"},
    "m_seq_lengths": "the reference serves m = 2 ... 16 (its docstring names fewer); anything else raises ValueError('Invalid length specified')",
    "deliberate_differences": {
        "seed": "cpx_awgn, cpx_awgn2 and awgn_channel take seed=None as a last argument.  The normals are the library's counter-based stream "
                "(Philox4x32-10, key = seed; row 0 from index 0) and never numpy.random.randn's values; seed=None takes 64 bits from NumPy's "
                "global generator (np.random.bytes(8)), so a script that calls np.random.seed stays reproducible.",
        "empty_input": "an empty x gives an empty array of the result dtype without a warning (the reference warns about the variance of an "
                       "empty slice); pn_gen(0) gives an empty float64 array.",
        "dtype": "float32 / complex64 in gives complex64 out, everything else complex128 (the reference always returns complex128).",
        "float32_rounding": "for complex64 output the variance, g x and sigma z and their sum are formed in float64 from the exactly widened "
                            "input and the sum is rounded ONCE to float32: the fixtures of complex64 cases hold the reference's result on "
                            "the widened input, and the library's equals it rounded to complex64 up to one float32 unit of the largest value.",
        "uint8_rows": "the *_rows forms that produce bits (random_bits_rows, pn_rows, awgn_channel_rows) return uint8, one byte per bit; "
                      "awgn_channel_rows marks a sum of exactly zero as 2 and a sum that is not a number as 3, which awgn_channel turns into "
                      "the reference's 0.5 and nan.",
        "bits_only": "awgn_channel accepts a one-dimensional array of 0 / 1 values only (ValueError otherwise); the reference maps any number "
                     "v to 2 v - 1.",
        "variance": "np.var is the deterministic merge of partial moments of the Gray demapper's scale: it differs from NumPy's pairwise sum by "
                    "about 1e-13 relative.",
    },
}
with open(os.path.join(HERE, "g23_conventions.json"), "w") as f:
    json.dump(conventions, f, indent=1, sort_keys=True)
    f.write("\n")
print("g23: %d awgn cases, %d channel cases (least margin %.3g), %d pn cases" % (len(awgn), len(chan), min(c["margin"] for c in chan), len(pn)))
