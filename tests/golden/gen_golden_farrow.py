#!/usr/bin/env python3
"""G15: golden vectors of digitalcom.farrow_resample (digitalcom.py:53-235), captured by running the REAL reference in the
dev container (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_farrow.py

  g15_farrow.npz        inputs x_<dtype>_<n> and outputs y<k>; "cases" is a JSON list of {key, x, fs_old, fs_new, i_ord, alpha}
  g15_conventions.json  what the reference returns or raises for the edge cases of its argument conventions

Every (ratio, dtype, order) at lengths 3, 4, 5 and 17; two long inputs (2400 samples) per ratio, dtype and order rotating.
"""
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import digitalcom as dc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1515)

RATIOS = [(8, 18), (48000, 44100), (1, np.pi), (np.e, 1), (15, 14), (3, 3), (10, 9.999), (-8, -18)]
DTYPES = ["float32", "float64", "complex64", "complex128"]
ORDERS = [(3, 0.5), (2, 0.5), (2, 0.3), (1, 0.5)]
SHORT = [3, 4, 5, 17]
LONG = 2400

out, cases = {}, []
for dt in DTYPES:
    for n in SHORT + [LONG]:
        x = rng.standard_normal(n)
        if dt.startswith("complex"):
            x = x + 1j * rng.standard_normal(n)
        out["x_%s_%d" % (dt, n)] = x.astype(dt)


def capture(dt, n, fs_old, fs_new, i_ord, alpha):
    xk = "x_%s_%d" % (dt, n)
    y = dc.farrow_resample(out[xk], fs_old, fs_new, i_ord=i_ord, alpha=alpha)
    key = "y%d" % len(cases)
    out[key] = y
    cases.append({"key": key, "x": xk, "fs_old": float(fs_old), "fs_new": float(fs_new), "i_ord": i_ord, "alpha": alpha})


for ri, (fo, fn) in enumerate(RATIOS):
    for dt in DTYPES:
        for i_ord, alpha in ORDERS:
            for n in SHORT:
                capture(dt, n, fo, fn, i_ord, alpha)
    capture(DTYPES[ri % 4], LONG, fo, fn, *ORDERS[ri % 4])
    capture(DTYPES[(ri + 2) % 4], LONG, fo, fn, *ORDERS[(ri + 1) % 4])

out["cases"] = np.array(json.dumps(cases))
np.savez_compressed(os.path.join(HERE, "g15_farrow.npz"), **out)


# ---- argument conventions -----------------------------------------------------------------------------------------
def outcome(fn):
    try:
        y = fn()
        return {"len": int(len(y)), "dtype": str(y.dtype)}
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__}


x10 = np.arange(10.0)
conv = {
    "i_ord_0": outcome(lambda: dc.farrow_resample(x10, 8, 18, i_ord=0)),
    "i_ord_4": outcome(lambda: dc.farrow_resample(x10, 8, 18, i_ord=4)),
    "empty": outcome(lambda: dc.farrow_resample(np.zeros(0), 8, 18)),
    "len1": outcome(lambda: dc.farrow_resample(np.ones(1), 8, 18)),
    "len2": outcome(lambda: dc.farrow_resample(np.ones(2), 8, 18)),
    "len3": outcome(lambda: dc.farrow_resample(np.ones(3), 8, 18)),
    "fs_old_0": outcome(lambda: dc.farrow_resample(x10, 0, 18)),
    "fs_new_0": outcome(lambda: dc.farrow_resample(x10, 8, 0)),
    "fs_new_inf": outcome(lambda: dc.farrow_resample(x10, 8, float("inf"))),
    "both_negative": outcome(lambda: dc.farrow_resample(x10, -8, -18)),
    "fs_new_negative": outcome(lambda: dc.farrow_resample(x10, 8, -18)),
    "fs_old_negative": outcome(lambda: dc.farrow_resample(x10, -8, 18)),
    "list": outcome(lambda: dc.farrow_resample([1.0, 2.0, 3.0, 4.0, 5.0], 8, 18)),
    "int64": outcome(lambda: dc.farrow_resample(np.arange(10), 8, 18)),
    "float32": outcome(lambda: dc.farrow_resample(x10.astype(np.float32), 8, 18)),
    "complex64": outcome(lambda: dc.farrow_resample(x10.astype(np.complex64), 8, 18)),
}
with open(os.path.join(HERE, "g15_conventions.json"), "w") as f:
    json.dump(conv, f, indent=1, sort_keys=True)
    f.write("\n")
print("g15: %d cases, %d bytes" % (len(cases), os.path.getsize(os.path.join(HERE, "g15_farrow.npz"))))
