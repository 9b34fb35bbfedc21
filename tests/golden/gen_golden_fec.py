#!/usr/bin/env python3
"""G19: fec_conv.FECConv (fec_conv.py:117-712) decoder / encoder / puncturing results and argument conventions from the
REAL reference (data only).  The reference decodes a few hundred to a few thousand bits per second: the cases are short.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_fec.py

  g19_fec.npz           "cases": JSON list of decoder cases {key, G, depth, metric, quant_level, group, note, calls}; call i of
                        a case has <key>_x<i> (received values: int8 for hard, float16 for soft, float64 for unquant -- each
                        widened exactly to what the reference was given) and <key>_y<i> (decoded bits, uint8).  A case with
                        several calls ran them on ONE object (the reference carries its trellis state from call to call).
                        "host": JSON list of conv_encoder / puncture / depuncture cases with <key>_in, <key>_out.
  g19_conventions.json  signatures, what unusual input returns or raises, the deliberate differences, and the reference's
                        measured decode rate per constraint length (ref_bits_per_s: a recorded result, no test threshold)
"""
import inspect
import json
import os
import sys
import time
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import fec_conv as fc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1919)

HALF = {3: ('111', '101'), 4: ('1111', '1101'), 5: ('11101', '10011'), 6: ('111101', '101011'), 7: ('1111001', '1011011'),
        8: ('11111001', '10100111'), 9: ('111101011', '101110001')}
THIRD = {3: ('111', '111', '101'), 4: ('1111', '1101', '1011'), 5: ('11111', '11011', '10101'), 6: ('111101', '101011', '100111'),
         7: ('1111001', '1100101', '1011011'), 8: ('11110111', '11011001', '10010101')}
DEPTH = {3: 10, 4: 20, 5: 25, 6: 30, 7: 35, 8: 40, 9: 45}

out, cases, host = {}, [], []
ref_rate = {}


def encode(G, bits):
    cc = fc.FECConv(G, 10)
    return cc.conv_encoder(bits, '0' * (len(G[0]) - 1))[0]


def widen(x):
    """what the reference is handed for a stored array: integers stay integers, floats become float64 (exact)"""
    return x.astype(np.int64) if x.dtype.kind == 'i' else x.astype(np.float64)


def capture(key, G, depth, metric, q, xs, group, note=""):
    """one object, one viterbi_decoder call per entry of xs"""
    cc = fc.FECConv(G, depth)
    t = 0.0
    nbits = 0
    for i, x in enumerate(xs):
        t0 = time.perf_counter()
        y = cc.viterbi_decoder(widen(x), metric, q)
        t += time.perf_counter() - t0
        assert y.dtype == np.float64 and np.all((y == 0) | (y == 1))
        out["%s_x%d" % (key, i)] = x
        out["%s_y%d" % (key, i)] = y.astype(np.uint8)
        nbits += len(y)
    cases.append({"key": key, "G": list(G), "depth": depth, "metric": metric, "quant_level": q, "group": group, "note": note,
                  "calls": len(xs)})
    return nbits, t


def soft_rx(code, sigma, q):
    """soft values centred on 0 and 2^q - 1, with fractional parts, some below 0 and some above the top level (float16 grid)"""
    top = 2 ** q - 1
    v = ((2 * code - 1) + sigma * rng.standard_normal(len(code)) + 1) / 2 * top
    return v.astype(np.float16)


def sigma_of(G):
    return (0.75 + 0.05 * len(G[0])) * (1.25 if len(G) == 3 else 1.0)


# ---- codes: every polynomial set of the constructor's docstring, soft, noisy -------------------------------------------
for rate, table in (("h", HALF), ("t", THIRD)):
    for K, G in table.items():
        msg = rng.integers(0, 2, 300)
        x = soft_rx(encode(G, msg), sigma_of(G), 3)
        nbits, t = capture("code_%s%d" % (rate, K), G, DEPTH[K], "soft", 3, [x], "codes")
        errs = int(np.sum(out["code_%s%d_y0" % (rate, K)] != msg[:nbits]))
        cases[-1]["note"] = "%d of %d decoded bits differ from the message" % (errs, nbits)
        if rate == "h":
            ref_rate[str(K)] = round(nbits / t, 1)

# ---- metrics: K = 3, 5, 7 at both rates ----------------------------------------------------------------------------------
for rate, table in (("h", HALF), ("t", THIRD)):
    for K in (3, 5, 7):
        G, D = table[K], DEPTH[K]
        tag = "%s%d" % (rate, K)
        msg = rng.integers(0, 2, 300)
        code = encode(G, msg)
        sg = sigma_of(G)
        hard = ((np.sign((2 * code - 1) + sg * rng.standard_normal(len(code))) + 1) / 2).astype(np.int8)
        capture("met_hard_" + tag, G, D, "hard", 3, [hard], "metrics")
        for q in (1, 3, 6):
            capture("met_soft%d_%s" % (q, tag), G, D, "soft", q, [soft_rx(code, sg, q)], "metrics")
        if rate == "h":   # punctured to rate 3/4 and de-punctured: every third value of each stream is the 3.5 erasure
            cc = fc.FECConv(G, D)
            rx = soft_rx(cc.puncture(code, ('110', '101')), 0.5, 3).astype(np.float64)
            dp = cc.depuncture(rx, ('110', '101'), 3.5)
            assert np.sum(dp == 3.5) == len(dp) // 3
            capture("met_depunct_" + tag, G, D, "soft", 3, [dp.astype(np.float16)], "metrics", "3.5 erasures count as 3")
        grid = np.round(((2 * code - 1) + sg * rng.standard_normal(len(code)) + 1) / 2 * 64) / 64
        capture("met_unq_grid_" + tag, G, D, "unquant", 3, [grid.astype(np.float64)], "metrics", "values on a grid of 1/64: every square and sum exact")
        gauss = ((2 * code - 1) + sg * rng.standard_normal(len(code)) + 1) / 2
        capture("met_unq_gauss_" + tag, G, D, "unquant", 3, [gauss.astype(np.float64)], "metrics", "continuous noise: the sums round")

# ---- depths ----------------------------------------------------------------------------------------------------------------
for K in (3, 7):
    for D in (1, 2, 10, 31, 32, 33, 63, 64, 65, 100, 128):
        G = HALF[K]
        msg = rng.integers(0, 2, 150 + D)
        capture("depth_h%d_%d" % (K, D), G, D, "soft", 3, [soft_rx(encode(G, msg), sigma_of(G), 3)], "depths")

# ---- ties: hard input where almost every comparison is a tie -----------------------------------------------------------------
for K in (3, 7):
    G, D = HALF[K], DEPTH[K]
    n = 2 * (120 + D)
    capture("tie_zero_h%d" % K, G, D, "hard", 3, [np.zeros(n, np.int8)], "ties")
    capture("tie_one_h%d" % K, G, D, "hard", 3, [np.ones(n, np.int8)], "ties")
    capture("tie_alt_h%d" % K, G, D, "hard", 3, [(np.arange(n) % 2).astype(np.int8)], "ties")
    capture("tie_clean_h%d" % K, G, D, "hard", 3, [encode(G, rng.integers(0, 2, n // 2)).astype(np.int8)], "ties")
G = THIRD[5]
capture("tie_zero_t5", G, 25, "hard", 3, [np.zeros(3 * 150, np.int8)], "ties")

# ---- state carry: three calls on one object, the second too short to emit anything --------------------------------------------
for rate, table, K in (("h", HALF, 3), ("h", HALF, 7), ("t", THIRD, 5), ("h", HALF, 9)):
    G, D = table[K], DEPTH[K]
    R = len(G)
    lens = (D + 60, D - 3, D + 101)          # symbols; R (D - 3) >= D values, which the reference needs to size its output
    xs = [soft_rx(encode(G, rng.integers(0, 2, L)), sigma_of(G), 3) for L in lens]
    capture("carry_soft_%s%d" % (rate, K), G, D, "soft", 3, xs, "carry")
G, D = HALF[7], 35
xs = [((2 * encode(G, rng.integers(0, 2, L)) - 1 + 0.9 * rng.standard_normal(2 * L) + 1) / 2).astype(np.float64) for L in (80, 33, 120)]
capture("carry_unq_h7", G, D, "unquant", 3, xs, "carry")
xs = [rng.integers(0, 2, 2 * L).astype(np.int8) for L in (70, 32, 90)]
capture("carry_hard_h7", G, D, "hard", 3, xs, "carry", "random bits: no code word anywhere near")

# ---- lengths -----------------------------------------------------------------------------------------------------------------
for rate, table, K in (("h", HALF, 3), ("h", HALF, 7), ("t", THIRD, 4), ("h", HALF, 8)):
    G, D = table[K], DEPTH[K]
    # D - 1 symbols: no output; then 1 and 2 outputs; 63 / 64 / 65 and 127 / 128 / 129 outputs (the output burst); symbol counts around
    # multiples of 16 and 64 (the symbol-load blocks)
    for nsym in sorted({D - 1, D, D + 1, D + 62, D + 63, D + 64, D + 126, D + 127, D + 128, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193}):
        if nsym * len(G) < D:
            continue
        x = soft_rx(encode(G, rng.integers(0, 2, nsym)), sigma_of(G), 3)
        capture("len_%s%d_%d" % (rate, K, nsym), G, D, "soft", 3, [x], "lengths")
for rate, table, K, nval in (("h", HALF, 3, 61), ("t", THIRD, 5, 100), ("t", THIRD, 5, 101), ("h", HALF, 7, 141)):
    G, D = table[K], DEPTH[K]
    capture("len_hard_ragged_%s%d_%d" % (rate, K, nval), G, D, "hard", 3, [rng.integers(0, 2, nval).astype(np.int8)], "lengths",
            "a value count that is no multiple of the rate denominator: hard takes the short last symbol as it is")

out["cases"] = np.array(json.dumps(cases))


# ---- host functions ------------------------------------------------------------------------------------------------------------
def with_warnings(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = fn()
    return r, [str(v.message) for v in w]


for rate, table, K, state in (("h", HALF, 3, '00'), ("h", HALF, 3, '10'), ("h", HALF, 7, '000000'), ("h", HALF, 7, '101101'),
                              ("t", THIRD, 3, '01'), ("t", THIRD, 5, '0000'), ("t", THIRD, 8, '1100101'), ("h", HALF, 9, '00110011')):
    G = table[K]
    cc = fc.FECConv(G, 10)
    bits = rng.integers(0, 2, 97)
    y, s = cc.conv_encoder(bits, state)
    key = "enc_%s%d_%s" % (rate, K, state)
    out[key + "_in"], out[key + "_out"] = bits.astype(np.int8), np.asarray(y, np.float64)
    host.append({"key": key, "fn": "conv_encoder", "G": list(G), "state": state, "state_out": s, "out_dtype": str(np.asarray(y).dtype)})
cc = fc.FECConv(HALF[3], 10)
for fn, pat, n in (("puncture", ('110', '101'), 60), ("puncture", ('1101', '1011'), 64), ("puncture", ('110', '101'), 61), ("puncture", ('110', '101'), 64),
                   ("puncture", ('110', '101'), 63),
                   ("depuncture", ('110', '101'), 40), ("depuncture", ('1101', '1011'), 36), ("depuncture", ('110', '101'), 41), ("depuncture", ('110', '101'), 42),
                   ("depuncture", ('110', '101'), 43)):
    v = rng.integers(0, 2, n).astype(np.float64) if fn == "puncture" else np.round(rng.uniform(-1, 8, n) * 8) / 8
    y, w = with_warnings(lambda: getattr(cc, fn)(v, pat))
    key = "%s_%s_%d" % (fn[:3], pat[0], n)
    out[key + "_in"], out[key + "_out"] = v, np.asarray(y)
    host.append({"key": key, "fn": fn, "pattern": list(pat), "warnings": w, "out_dtype": str(np.asarray(y).dtype)})
v = np.round(rng.uniform(-1, 8, 40) * 8) / 8
out["dep_erase_in"], out["dep_erase_out"] = v, cc.depuncture(v, ('110', '101'), -2.25)
host.append({"key": "dep_erase", "fn": "depuncture", "pattern": ['110', '101'], "erase_value": -2.25, "warnings": [], "out_dtype": "float64"})
out["host"] = np.array(json.dumps(host))
np.savez_compressed(os.path.join(HERE, "g19_fec.npz"), **out)


# ---- argument conventions ----------------------------------------------------------------------------------------------------------
def outcome(fn):
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            y = fn()
        y = np.asarray(y)
        return {"shape": list(y.shape), "dtype": str(y.dtype), "warnings": sorted({str(v.message) for v in w})}
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__, "message": str(e)}


def dec(x, metric='soft', q=3, G=HALF[3], D=10):
    return lambda: fc.FECConv(G, D).viterbi_decoder(x, metric, q)


xs = np.round(rng.uniform(0, 7, 60) * 4) / 4
xb = rng.integers(0, 2, 60)
xnan = xs.copy()
xnan[7] = np.nan
xinf = xs.copy()
xinf[7] = np.inf
conv = {
    "signatures": {name: [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(getattr(fc.FECConv, name)).parameters.values()]
                   for name in ("__init__", "viterbi_decoder", "conv_encoder", "puncture", "depuncture", "trellis_plot", "traceback_plot")},
    "decoder": {},
    "one_poly": outcome(lambda: fc.FECConv(('111',), 10)),
    "four_polys": outcome(lambda: fc.FECConv(('111', '101', '110', '011'), 10)),
    "bad_metric": outcome(dec(xs, 'euclid')),
    "hard_float": outcome(dec(xb.astype(np.float64), 'hard')),
    "hard_value_2": outcome(dec(np.where(np.arange(60) == 5, 2, xb), 'hard')),
    "hard_negative": outcome(dec(np.where(np.arange(60) == 5, -1, xb), 'hard')),
    "soft_nan": outcome(dec(xnan)),
    "soft_inf": outcome(dec(xinf)),
    "unquant_nan": outcome(dec(xnan, 'unquant')),
    "soft_odd_count": outcome(dec(xs[:59])),
    "unquant_odd_count": outcome(dec(xs[:59], 'unquant')),
    "hard_odd_count": outcome(dec(xb[:59], 'hard')),
    "fewer_values_than_depth": outcome(dec(xs[:8])),
    "ref_bits_per_s": ref_rate,
    "ref_bits_per_s_note": "rate 1/2, soft, 300-bit frames, decision depth 10/20/25/30/35/40/45 for K = 3 ... 9, one CPU core, at generation time",
    "deliberate_differences": {
        "cumulative_metric": "paths.cumulative_metric (and traceback_states / traceback_bits) are not mirrored: the hard and soft metrics are kept "
                             "normalised (the step's minimum subtracted), which leaves every decision and every output bit unchanged",
        "non_finite": "soft / unquant input holding nan or inf raises ValueError; the reference raises ValueError (nan) or OverflowError (inf) from int() "
                      "for soft and silently mis-compares for unquant",
        "x_2d": "2-D input to viterbi_decoder raises ValueError pointing at viterbi_decoder_rows; the reference takes rows for values and fails or "
                "returns nonsense",
        "soft_range": "soft: |int(x)| <= 4095 and 0 <= quant_level <= 12 (the 32-bit metrics' headroom), else ValueError; the reference takes any size",
        "metric_family": "a call whose metric_type changes between hard / soft and unquant on an object that is not at rest raises ValueError (reset() "
                         "first): the carried metrics of one family are not those of the other; the reference carries them over as they are",
        "containers": "lists and tuples are accepted wherever an array is (the reference needs x.dtype for hard); unsigned integer arrays decode as their "
                      "values (the reference's abs(x - bit) wraps for them)",
        "encoder_input": "conv_encoder takes bits 0 / 1 only (ValueError otherwise) and returns an empty float64 array for empty input; the reference "
                         "XORs whatever int() gives and returns an empty list",
        "plots": "trellis_plot / traceback_plot are out of scope",
    },
}
for name, x in (("list", list(xs)), ("tuple", tuple(xs)), ("float32", xs.astype(np.float32)), ("int64", xs.astype(np.int64)),
                ("two_d", xs.reshape(2, 30)), ("empty", np.zeros(0))):
    conv["decoder"][name] = {m: outcome(dec(x, m)) for m in ("soft", "unquant")}
for name, x in (("list", list(xb)), ("tuple", tuple(xb)), ("int64", xb.astype(np.int64)), ("int8", xb.astype(np.int8)), ("two_d", xb.reshape(2, 30)),
                ("empty", np.zeros(0, np.int64))):
    conv["decoder"][name] = dict(conv["decoder"].get(name, {}), hard=outcome(dec(x, "hard")))
with open(os.path.join(HERE, "g19_conventions.json"), "w") as fh:
    json.dump(conv, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("g19: %d decoder cases, %d host cases, %d bytes; reference bits/s %s" % (len(cases), len(host), os.path.getsize(os.path.join(HERE, "g19_fec.npz")), ref_rate))
