#!/usr/bin/env python3
"""G20: fec_block.FECHamming / FECCyclic (fec_block.py:61-423) encoder / decoder results and argument conventions from the REAL
reference (data only).  The reference decodes 0.1 - 1 Mbit/s (Hamming) and a few kbit/s (cyclic): the cases are short.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_fecblock.py

  g20_fecblock.npz      "cases": JSON list {key, kind ("hamming" | "cyclic"), j, G (cyclic), fn ("encode" | "decode"), group, nin, nout,
                        in_dtype, out_dtype}; <key>_in and <key>_out are the bits the reference was given (as int64) and returned,
                        stored with np.packbits (nin / nout are the bit counts).
  g20_conventions.json  signatures, return dtypes, what unusual input returns or raises, the deliberate differences, and the
                        reference's measured decode rate per code (ref_bits_per_s: a recorded result, no test threshold)
"""
import inspect
import json
import os
import sys
import time

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import fec_block as fb  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(2020)

DOC_G = {3: '1011', 4: '10011', 5: '101001', 6: '1100001', 7: '10100001', 8: '101110001'}
NONPRIMITIVE = ('1001', '11111', '100001', '1110101')
OTHER = ('1101',)

out, cases = {}, []
ref_rate = {}


def store(key, kind, j, G, fn, group, x, y):
    y = np.asarray(y)
    assert np.all((y == 0) | (y == 1))
    out[key + "_in"], out[key + "_out"] = np.packbits(x.astype(np.uint8)), np.packbits(y.astype(np.uint8))
    cases.append({"key": key, "kind": kind, "j": j, "G": G, "fn": fn, "group": group, "nin": int(x.size), "nout": int(y.size),
                  "in_dtype": str(x.dtype), "out_dtype": str(y.dtype)})


def flipped(code, n, positions):
    """block b of `code` with positions[b] (a list) flipped"""
    c = code.copy().reshape(-1, n)
    for b, pos in enumerate(positions):
        for q in pos:
            c[b, q] ^= 1
    return c.reshape(-1)


def capture(tag, kind, j, G, enc, dec, nblk):
    n = 2 ** j - 1
    k = n - j
    x = rng.integers(0, 2, nblk * k)
    code = np.asarray(enc(x))
    store(tag + "_enc", kind, j, G, "encode", "encode", x, code)
    code = code.astype(np.int64)
    if n <= 63:
        single = list(range(n))
    else:
        single = sorted({0, 1, k - 1, k, n - 1} | set(int(v) for v in rng.choice(n, 20, replace=False)))
    groups = [("clean", code)]
    # n <= 63: a code word of its own per flipped position; beyond: the first code word again and again
    base = np.asarray(enc(rng.integers(0, 2, len(single) * k))).astype(np.int64) if n <= 63 else np.tile(code[:n], len(single))
    groups.append(("one_error", flipped(base, n, [[q] for q in single])))
    groups.append(("two_errors", flipped(code, n, [list(rng.choice(n, 2, replace=False)) for _ in range(nblk)])))
    groups.append(("three_errors", flipped(code, n, [list(rng.choice(n, 3, replace=False)) for _ in range(nblk)])))
    groups.append(("random", rng.integers(0, 2, nblk * n)))
    t, bits = 0.0, 0
    for group, c in groups:
        t0 = time.perf_counter()
        y = dec(c.copy())   # (hamm_decoder corrects the array it is given in place)
        t += time.perf_counter() - t0
        bits += len(y)
        store("%s_%s" % (tag, group), kind, j, G, "decode", group, c, y)
    ref_rate[tag] = round(bits / t)


for j in (3, 4, 5, 6, 7, 8, 10):
    h = fb.FECHamming(j)
    capture("ham%d" % j, "hamming", j, None, h.hamm_encoder, h.hamm_decoder, {3: 40, 4: 40, 5: 30, 6: 20, 7: 12, 8: 8, 10: 4}[j])
for G in list(DOC_G.values()) + list(NONPRIMITIVE) + list(OTHER):
    c = fb.FECCyclic(G)
    j = len(G) - 1
    capture("cyc" + G, "cyclic", j, G, c.cyclic_encoder, c.cyclic_decoder, {3: 24, 4: 16, 5: 10, 6: 6, 7: 4, 8: 3}[j])
out["cases"] = np.array(json.dumps(cases))
np.savez_compressed(os.path.join(HERE, "g20_fecblock.npz"), **out)


# ---- argument conventions ----------------------------------------------------------------------------------------------------------
def outcome(fn):
    try:
        y = np.asarray(fn())
        return {"shape": list(y.shape), "dtype": str(y.dtype)}
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__, "message": str(e)}


def sig(cls, name):
    return [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(getattr(cls, name)).parameters.values()]


ham, cyc = fb.FECHamming(3), fb.FECCyclic('1011')
x4 = rng.integers(0, 2, 8)
c7 = ham.hamm_encoder(x4).astype(int)
methods = {"hamm_encoder": (ham.hamm_encoder, x4, 4), "hamm_decoder": (ham.hamm_decoder, c7, 7),
           "cyclic_encoder": (cyc.cyclic_encoder, x4, 4), "cyclic_decoder": (cyc.cyclic_decoder, c7, 7)}
conv = {
    "signatures": {"FECHamming": {name: sig(fb.FECHamming, name) for name in ("__init__", "hamm_gen", "hamm_encoder", "hamm_decoder")},
                   "FECCyclic": {name: sig(fb.FECCyclic, name) for name in ("__init__", "cyclic_encoder", "cyclic_decoder")}},
    "hamm_gen": {"types": [type(v).__name__ for v in ham.hamm_gen(3)], "dtypes": [str(v.dtype) for v in ham.hamm_gen(3)[:3]],
                 "shapes": [list(v.shape) for v in ham.hamm_gen(3)[:3]]},
    "methods": {},
    "hamming_j2": outcome(lambda: fb.FECHamming(2)),
    "cyclic_j2": outcome(lambda: fb.FECCyclic('111').cyclic_encoder(np.array([1]))),
    "cyclic_bad_first": outcome(lambda: fb.FECCyclic('0011')),
    "cyclic_bad_last": outcome(lambda: fb.FECCyclic('1010')),
    "cyclic_encoder_ignores_G": bool(np.array_equal(cyc.cyclic_encoder(x4, '1101'), cyc.cyclic_encoder(x4))),
    "ref_bits_per_s": ref_rate,
    "ref_bits_per_s_note": "decoded bits per second over the captured decoder cases of each code (calls of 3 - 63 blocks), one CPU core, at generation time",
    "deliberate_differences": {
        "j_range": "j = 3 ... 16 (n <= 65535) for both classes, else ValueError; the reference's hamm_gen takes any j >= 3 (34 GB of matrices at j = 16) "
                   "and FECCyclic any polynomial of two or more digits, j = 2 included (its loops take seconds per block from j = 12 on)",
        "bit_values": "bits must be 0 / 1, else ValueError; the reference reduces whatever it is given mod 2 (see methods.*.value_2 / negative)",
        "containers": "lists, tuples and every integer dtype are accepted; the reference compares np.dtype(x[0]) with int: it raises TypeError for a list "
                      "of Python ints and ValueError for int32 / uint8 (see methods.*.list / int32 / uint8)",
        "empty": "empty input returns an empty array of the method's dtype; the reference raises (see methods.*.empty)",
        "lazy_matrices": "FECHamming.G and .R are properties built on first use (133 MB each at j = 12); H, n, k, j are attributes as in the reference",
        "in_place": "hamm_decoder leaves the caller's array as it was; the reference corrects the code words in the array it is given",
        "bounds": "ser2ber and block_single_error_Pb_bound are out of scope",
    },
}
for name, (fn, good, per) in methods.items():
    conv["methods"][name] = {
        "good": outcome(lambda: fn(good)),
        "float": outcome(lambda: fn(good.astype(np.float64))),
        "bad_length": outcome(lambda: fn(good[:per + 1])),
        "short": outcome(lambda: fn(good[:per - 1])),
        "int32": outcome(lambda: fn(good.astype(np.int32))),
        "uint8": outcome(lambda: fn(good.astype(np.uint8))),
        "list": outcome(lambda: fn([int(v) for v in good])),
        "value_2": outcome(lambda: fn(np.where(np.arange(good.size) == 1, 2, good))),
        "negative": outcome(lambda: fn(np.where(np.arange(good.size) == 1, -1, good))),
        "empty": outcome(lambda: fn(np.zeros(0, dtype=int))),
    }
with open(os.path.join(HERE, "g20_conventions.json"), "w") as fh:
    json.dump(conv, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("g20: %d cases, %d bytes; reference bits/s %s" % (len(cases), os.path.getsize(os.path.join(HERE, "g20_fecblock.npz")), ref_rate))
