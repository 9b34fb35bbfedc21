#!/usr/bin/env python3
"""G22: Gray symbol mapping and demapping -- digitalcom.qam_gray_decode / mpsk_gray_decode (digitalcom.py:1684-1739, 1829-1883) and the symbol
sequences of qam_gray_encode_bb / mpsk_gray_encode_bb at ns = 1 (digitalcom.py:1584-1681, 1742-1826) -- results, dtypes, warnings and
failures from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_symmap.py

  g22_symmap.npz        "dec": JSON list of decode cases {key, fn, mod, tag, n, in_dtype, ref_in, out_dtype, margin}: <key>_in, <key>_out.
                        ref_in "same": the reference decoded <key>_in itself; "widened": it decoded <key>_in.astype(complex128).
                        margin: the least distance of any component (QAM: in level units, of (x / s + x_m (1 + 1j)) / 2 from the half-integers
                        strictly inside (0, x_m); MPSK: of angle * mod / 2 / pi from the half-integers), by the reference's own formula.
                        "spec": JSON list of {key, mod}: the exact specials of mpsk_gray_decode, <key>_in / <key>_out (margin 0: on thresholds).
                        "map": JSON list of mapper cases {key, fn, mod, nbits, n_symb, x_dtype, data_len}: <key>_bits (ext_data), <key>_x
                        (the symbols, complex128) -- ext_data lengths that are no multiple of the bits per symbol included.
  g22_conventions.json  signatures, how the reference treats an empty input and a bad order, the deliberate differences

The generator REFUSES to write a decode case whose margin is below its bound (1e-6; 2e-3 where the reference takes np.std in float32): no
fixture depends on which way a rounding error tips a decision.  No symbol is excluded from any comparison.
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

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(2222)
QAM = (2, 4, 16, 64, 256)
MPSK = (2, 4, 8, 16, 32)
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


def half_integer_distance(k, lo, hi):
    """the least distance of any k from the half-integers j + 0.5, lo <= j + 0.5 <= hi (inf where there is none)"""
    k = np.asarray(k, dtype=np.float64).reshape(-1)
    th = np.arange(np.ceil(lo - 0.5), np.floor(hi - 0.5) + 1) + 0.5
    th = th[(th > lo) & (th < hi)]
    if th.size == 0 or k.size == 0:
        return np.full(k.shape, np.inf)
    return np.min(np.abs(k[:, None] - th[None, :]), axis=1)


def qam_margins(x, mod):
    """per symbol, by the reference's own formula (np.std in x's own precision)"""
    x_m = 1 if mod == 2 else np.sqrt(mod) - 1
    xs = x / (np.std(x) * np.sqrt(3 / (2 * (mod - 1))))
    k = (xs + x_m * (1 + 1j)) / 2
    if mod == 2:                        # the quadrature component is not decided
        return half_integer_distance(k.real, 0, x_m)
    return np.minimum(half_integer_distance(k.real, 0, x_m), half_integer_distance(k.imag, 0, x_m))


def mpsk_margins(x, mod):
    if mod == 4:
        x = x * np.exp(-1j * np.pi / 4)
    v = np.angle(x) * mod / 2 / np.pi
    return np.abs(np.abs(v - np.floor(v)) - 0.5)


def noise(n, sigma):
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


dec = []


def add_dec(fn, mod, tag, x, ref_in, bound):
    ref_x = x.astype(np.complex128) if ref_in == "widened" else x
    margins = qam_margins(ref_x, mod) if fn == "qam_gray_decode" else mpsk_margins(ref_x, mod)
    margin = float(np.min(margins))
    if not margin >= bound:
        raise SystemExit("REFUSED %s mod %d %s: the least margin %.3g is below %.3g" % (fn, mod, tag, margin, bound))
    y = getattr(dc, fn)(ref_x, mod)
    key = "%s_%d_%s" % ("qd" if fn == "qam_gray_decode" else "pd", mod, tag)
    out[key + "_in"], out[key + "_out"] = x, np.asarray(y)
    dec.append({"key": key, "fn": fn, "mod": mod, "tag": tag, "n": int(x.size), "in_dtype": str(x.dtype), "ref_in": ref_in, "out_dtype": str(np.asarray(y).dtype),
                "out_type": type(y).__name__, "margin": margin, "bound": bound})


# ---- qam_gray_decode ---------------------------------------------------------------------------------------------------------
for mod in QAM:
    bps = int(np.log2(mod))
    n = {2: 257, 4: 300, 16: 1025, 64: 4096, 256: 2049}[mod]
    x = np.asarray(dc.qam_gray_encode_bb(None, 1, mod, ext_data=rng.integers(0, 2, n * bps))[0], dtype=np.complex128)
    sigma = 0.45 / (1 if mod == 2 else np.sqrt(mod) - 1)       # 0.45 of half the level spacing: symbol errors at every order
    add_dec("qam_gray_decode", mod, "clean", x, "same", 1e-6)
    noisy = x + noise(n, sigma)
    add_dec("qam_gray_decode", mod, "noisy", noisy, "same", 1e-6)
    add_dec("qam_gray_decode", mod, "offset", (0.7 - 0.2j) * noisy + (0.05 + 0.02j), "same", 1e-6)   # another gain and a small DC term: the adaptive scale at work
    # complex64: the reference on the widened array (what the device computes), and on the array itself (np.std in float32)
    x32 = noisy.astype(np.complex64)
    add_dec("qam_gray_decode", mod, "c64w", x32, "widened", 1e-6)
    x32 = x32[:512]                                              # few symbols to drop: the recomputed np.std barely moves
    keep = x32[qam_margins(x32, mod) >= 2e-3]
    add_dec("qam_gray_decode", mod, "c64", keep, "same", 2e-3)    # std recomputed on what is left: refused if the margin no longer holds
# real input (mod 2 accepts it in the reference; the other orders do as well)
xr = 2.0 * rng.integers(0, 2, 200) - 1 + 0.4 * rng.standard_normal(200)
add_dec("qam_gray_decode", 2, "real", xr, "same", 1e-6)

# ---- mpsk_gray_decode --------------------------------------------------------------------------------------------------------
spec = []
for mod in MPSK:
    bps = int(np.log2(mod))
    n = {2: 257, 4: 300, 8: 1025, 16: 4096, 32: 2049}[mod]
    x = np.asarray(dc.mpsk_gray_encode_bb(None, 1, mod, ext_data=rng.integers(0, 2, n * bps))[0], dtype=np.complex128)
    add_dec("mpsk_gray_decode", mod, "clean", x, "same", 1e-6)
    noisy = (x + noise(n, 0.45 * np.sin(np.pi / mod))) * rng.uniform(0.2, 5.0, n)      # the amplitude does not matter
    add_dec("mpsk_gray_decode", mod, "noisy", noisy, "same", 1e-6)
    add_dec("mpsk_gray_decode", mod, "c64w", noisy.astype(np.complex64), "widened", 1e-6)
    # the exact specials: 0, +-1, +-1j, -1 - 0j, purely real and purely imaginary values of either sign
    s = np.array([0, 1, -1, 1j, -1j, complex(-1.0, -0.0), 2.5, -0.3, 0.7j, -4j, complex(3.0, -0.0), complex(0.0, 0.0) * -1], dtype=np.complex128)
    key = "ps_%d" % mod
    out[key + "_in"], out[key + "_out"] = s, np.asarray(dc.mpsk_gray_decode(s, mod))
    spec.append({"key": key, "mod": mod})

# ---- the encoders' symbol sequences at ns = 1 -----------------------------------------------------------------------------------
maps = []
for fn, orders in (("qam_gray_encode_bb", QAM), ("mpsk_gray_encode_bb", MPSK)):
    for mod in orders:
        bps = int(np.log2(mod))
        for extra in sorted({0, 1, bps - 1}):                      # bits beyond the last whole symbol: the reference truncates
            nbits = (2 ** bps * 3 + 5) * bps + extra        # every word several times
            bits = rng.integers(0, 2, nbits)
            if extra == 0:                                  # ... and every word at least once, whatever the draw
                words = np.arange(2 ** bps)
                bits[:2 ** bps * bps] = ((words[:, None] >> np.arange(bps - 1, -1, -1)) & 1).reshape(-1)
            x, b, data = getattr(dc, fn)(None, 1, mod, ext_data=bits)
            key = "%s_%d_%d" % ("qm" if fn.startswith("qam") else "pm", mod, extra)
            out[key + "_bits"], out[key + "_x"] = bits.astype(np.uint8), np.asarray(x).astype(np.complex128)
            maps.append({"key": key, "fn": fn, "mod": mod, "nbits": nbits, "n_symb": int(len(x)), "x_dtype": str(np.asarray(x).dtype), "data_len": int(len(data)),
                         "b": b if isinstance(b, int) else None})

out["dec"], out["spec"], out["map"] = np.array(json.dumps(dec)), np.array(json.dumps(spec)), np.array(json.dumps(maps))
np.savez_compressed(os.path.join(HERE, "g22_symmap.npz"), **out)

# ---- conventions -----------------------------------------------------------------------------------------------------------------
e128 = np.zeros(0, dtype=np.complex128)
one = np.ones(5, dtype=np.complex128)
conv = {
    "signatures": {fn: str(inspect.signature(getattr(dc, fn))) for fn in ("qam_gray_decode", "mpsk_gray_decode", "qam_gray_encode_bb", "mpsk_gray_encode_bb")},
    "empty input": {"qam_gray_decode mod %d" % m: outcome(lambda m=m: dc.qam_gray_decode(e128, m)) for m in (2, 4, 16)},
    "bad order": {"qam_gray_decode mod 8": outcome(lambda: dc.qam_gray_decode(one + 1j * np.arange(5), 8)),
                  "mpsk_gray_decode mod 64": outcome(lambda: dc.mpsk_gray_decode(one, 64)),
                  "qam_gray_decode mod 8, empty": outcome(lambda: dc.qam_gray_decode(e128, 8)),
                  "mpsk_gray_decode mod 64, empty": outcome(lambda: dc.mpsk_gray_decode(e128, 64))},
    "all-equal frame": {"qam_gray_decode mod 4": outcome(lambda: dc.qam_gray_decode(one, 4))},
    "deliberate differences": [
        "a bad order raises the reference's ValueError text for an empty x_hat too (the reference raises inside its loop over the symbols, so not for an empty input)",
        "len(x_hat) == 0 returns an empty int64 array (mod 2 as well: the reference's loop never runs) without a launch and without the reference's warnings",
        "a QAM scale that is zero, NaN or infinite (an all-equal frame, a non-finite sample) raises ValueError; the reference divides by it and casts NaN to an integer, which is platform-defined. "
        "The public functions read the scale back and check it; the _dev forms leave it on the device and do not check it",
        "real-valued input is widened to complex (the reference then divides by s where it multiplies a complex array by 1 / s: at most one ulp, visible on a threshold only)",
        "integer input runs as float64",
        "float32 / complex64 input is widened exactly and decided in float64 (the reference takes np.std and np.angle in float32)",
        "qam_gray_map_rows / mpsk_gray_map_rows always return complex symbols (the reference's mod 2 sequences are float64 resp. int64 arrays 2 * data - 1)",
        "the *_rows forms (beyond the reference) return uint8, one row per frame",
    ],
}
conv["empty input"].update({"mpsk_gray_decode mod %d" % m: outcome(lambda m=m: dc.mpsk_gray_decode(e128, m)) for m in (2, 4, 8)})
with open(os.path.join(HERE, "g22_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("g22: %d decode cases (least margin %.3g), %d special sets, %d mapper cases" % (len(dec), min(d["margin"] for d in dec), len(spec), len(maps)))
