#!/usr/bin/env python3
"""G17: sigsys.fft_caf (sigsys.py:2696-2781) outputs and argument conventions from the REAL reference (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_caf.py

  g17_caf.npz           per case <key>_x, <key>_h (inputs), <key>_y, <key>_f, <key>_t (the three results) and <key>_out (the
                        printed lines); "cases" is a JSON list of {key, args, note}
  g17_conventions.json  what the reference returns or raises for list, integer, short and 2-D input and for a reference
                        waveform longer than n_fft2
"""
import contextlib
import io
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import sigsys as ss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1717)


def noise(n, cplx):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


out, cases = {}, []


def capture(key, x, h, note, **args):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        y, f, t = ss.fft_caf(x, h, **args)
    out.update({key + "_x": x, key + "_h": h, key + "_y": y, key + "_f": f, key + "_t": t, key + "_out": np.array(buf.getvalue())})
    cases.append({"key": key, "args": args, "note": note})


capture("real300", noise(2500, False), noise(300, False), "real input, 7 slices, two blocks and a tail of 500",
        n_fft2=1000, n_slice2=3, bs=0.5, fs=1000.0)
capture("cplx65", noise(1000, True), noise(65, False), "complex input, 5 slices, 1000 = 7 * 128 + 104",
        n_fft2=128, n_slice2=2, bs=20.0, fs=1000.0)
capture("full2049", noise(4500, True), noise(2049, False), "len(h_ref) = n_fft2 = 2049, step = 1229",
        n_fft2=2049, n_slice2=1, bs=0.3, fs=1.0)
capture("wrap100", noise(450, True), noise(40, False), "step = 60, n_slice2 = 4: shifts up to +-240 exceed 2 * n_fft2 = 200 and wrap",
        n_fft2=100, n_slice2=4, bs=0.3, fs=1.0)
capture("slice0", noise(700, False), noise(50, False), "n_slice2 = 0 (the default): one slice", n_fft2=256)
capture("onetap", noise(600, True), np.array([0.75]), "len(h_ref) = 1", n_fft2=64, n_slice2=1, bs=0.25, fs=2.0)
capture("cplxref", noise(900, True), noise(33, True), "complex h_ref", n_fft2=200, n_slice2=2, bs=12.5, fs=500.0)
capture("ragged", noise(777, False), noise(100, False), "len(x) = 777 = 7 * 100 + 77, len(h_ref) = n_fft2", n_fft2=100, n_slice2=1, bs=1.0, fs=10.0)

out["cases"] = np.array(json.dumps(cases))
np.savez_compressed(os.path.join(HERE, "g17_caf.npz"), **out)


# ---- argument conventions -----------------------------------------------------------------------------------------
def outcome(fn):
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            y, f, t = fn()
        r = {"stdout": buf.getvalue()}
        for name, v in (("y", y), ("f", f), ("t", t)):
            v = np.asarray(v)
            r[name] = {"shape": list(v.shape), "dtype": str(v.dtype), "all_zero": bool(v.size and not np.any(v))}
        return r
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__, "message": str(e)}


xr = rng.standard_normal(600)
h = rng.standard_normal(20)
conv = {
    "signature": [[p.name, None if p.default is p.empty else p.default]
                  for p in __import__("inspect").signature(ss.fft_caf).parameters.values()],
    "x_list": outcome(lambda: ss.fft_caf(list(xr), h, n_fft2=64)),
    "x_tuple": outcome(lambda: ss.fft_caf(tuple(xr), h, n_fft2=64)),
    "x_list_short": outcome(lambda: ss.fft_caf(list(xr[:50]), h, n_fft2=64)),
    "x_short": outcome(lambda: ss.fft_caf(xr[:50], h, n_fft2=64, n_slice2=1)),
    "x_empty": outcome(lambda: ss.fft_caf(np.zeros(0), h, n_fft2=64)),
    "x_int64": outcome(lambda: ss.fft_caf(np.arange(600) % 17, h, n_fft2=64)),
    "x_float32": outcome(lambda: ss.fft_caf(xr.astype(np.float32), h, n_fft2=64)),
    "x_2d": outcome(lambda: ss.fft_caf(xr.reshape(2, 300), h, n_fft2=64)),
    "h_list": outcome(lambda: ss.fft_caf(xr, list(h), n_fft2=64)),
    "h_int64": outcome(lambda: ss.fft_caf(xr, np.arange(20) % 5, n_fft2=64)),
    "h_too_long": outcome(lambda: ss.fft_caf(xr, h, n_fft2=19)),
    "deliberate_differences": {
        "x_2d": "the reference counts rows as samples and returns a meaningless (slices, rows) array; here ValueError: x_in must be one-dimensional",
        "non_finite": "the reference's FFT form spreads an inf / nan sample over the whole 2 n_fft2 block of every slice; here it stays inside the "
                      "len(h_ref) outputs per row that multiply it",
    },
}
with open(os.path.join(HERE, "g17_conventions.json"), "w") as fh:
    json.dump(conv, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("g17: %d cases, %d bytes" % (len(cases), os.path.getsize(os.path.join(HERE, "g17_caf.npz"))))
