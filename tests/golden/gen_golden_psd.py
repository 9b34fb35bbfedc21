#!/usr/bin/env python3
"""G16: golden vectors of sigsys.psd / sigsys.my_psd / digitalcom.my_psd / sigsys.simple_sa (sigsys.py:2497-2585, 2457-2494,
1008-1084; digitalcom.py:1051-1086), captured by running the REAL reference in the dev container (data only).

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_psd.py

  g16_psd.npz           "x": 20000 complex128 samples (noise plus two tones); every case runs on a prefix of it cast to the
                        case's dtype (real dtypes take the real part: x_of below); outputs <key> (the spectrum) and <key>_f
                        (the frequency axis); "cases" is a JSON list of {key, fn, dtype, Q, args}
  g16_conventions.json  what the reference returns or raises for list, integer and 2-D input, K = 0 and NAVG > K

psd: every (dtype, n_fft) at 20000 samples with overlap and scaling rotating; every (overlap, scale_noise, dtype) at
n_fft = 256; the lengths n_fft, n_fft + 1, n_fft + step, n_fft + step + 1 (K = 0, 1, 1, 2) for every n_fft.
"""
import json
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from sk_dsp_comm import sigsys as ss  # noqa: E402
from sk_dsp_comm import digitalcom as dc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(1616)

DTYPES = ["float32", "float64", "complex64", "complex128"]
NFFTS = [64, 256, 1024, 4096, 1000]
OVERLAPS = [0, 37, 50, 75]
LONG = 20000

m = np.arange(LONG)
x = (rng.standard_normal(LONG) + 1j * rng.standard_normal(LONG)) / np.sqrt(2)
x = x + 3 * np.exp(2j * np.pi * 0.125 * m) + 0.5 * np.cos(2 * np.pi * 0.3017 * m)
out, cases = {"x": x}, []


def x_of(dtype, Q):
    v = x[:Q]
    return (v if dtype.startswith("complex") else v.real).astype(dtype)


def capture(fn, dtype, Q, **args):
    xin = x_of(dtype, Q)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if fn == "psd":
            P, f = ss.psd(xin, **args)
        elif fn == "my_psd":
            P, f = ss.my_psd(xin, **args)
        elif fn == "dc_my_psd":
            P, f = dc.my_psd(xin, **args)
        else:
            f, P = ss.simple_sa(xin, **args)
    key = "y%d" % len(cases)
    out[key] = P
    out[key + "_f"] = f
    cases.append({"key": key, "fn": fn, "dtype": dtype, "Q": Q, "args": args})


rot = 0
for dt in DTYPES:
    for n_fft in NFFTS:
        capture("psd", dt, LONG, n_fft=n_fft, fs=1 + rot % 3, overlap_percent=OVERLAPS[rot % 4], scale_noise=bool(rot % 2 == 0))
        rot += 1
for dt in DTYPES:
    for ov in OVERLAPS:
        for sn in (True, False):
            capture("psd", dt, LONG, n_fft=256, fs=1, overlap_percent=ov, scale_noise=sn)
for n_fft in NFFTS:
    for li in range(4):
        ov = OVERLAPS[(rot + li) % 4]
        step = n_fft - int(np.round(ov / 100 * n_fft))
        Q = [n_fft, n_fft + 1, n_fft + step, n_fft + step + 1][li]
        capture("psd", DTYPES[(rot + li) % 4], Q, n_fft=n_fft, fs=2, overlap_percent=ov, scale_noise=bool((rot + li) % 2))
        if n_fft <= 1024:
            capture("psd", DTYPES[(rot + li + 2) % 4], Q, n_fft=n_fft, fs=1, overlap_percent=50, scale_noise=True)
    rot += 1

for dt in DTYPES:
    capture("my_psd", dt, 700, n_fft=1024, fs=1)
    capture("my_psd", dt, LONG, n_fft=1024, fs=10)
    capture("my_psd", dt, LONG, n_fft=1000, fs=1)
    capture("my_psd", dt, 5000, n_fft=64, fs=2)
    capture("my_psd", dt, 3001, n_fft=255, fs=1)
    capture("dc_my_psd", dt, 9000, NFFT=256, Fs=4)

for dt in DTYPES:
    capture("simple_sa", dt, 2048, NS=128, NFFT=512, fs=10000)
    capture("simple_sa", dt, LONG, NS=128, NFFT=512, fs=10000, NAVG=5, window="hann")
    capture("simple_sa", dt, LONG, NS=256, NFFT=256, fs=1, NAVG=7, window="boxcar")
    capture("simple_sa", dt, LONG, NS=1024, NFFT=1024, fs=1, NAVG=3, window="hann")
    capture("simple_sa", dt, 4000, NS=100, NFFT=1000, fs=8, NAVG=2, window="hann")

out["cases"] = np.array(json.dumps(cases))
np.savez_compressed(os.path.join(HERE, "g16_psd.npz"), **out)


# ---- argument conventions -----------------------------------------------------------------------------------------
def outcome(fn):
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            a, b = fn()
        r = {}
        for name, v in (("first", a), ("second", b)):
            v = np.asarray(v)
            r[name] = {"shape": list(v.shape), "dtype": str(v.dtype), "all_nan": bool(v.size and np.all(np.isnan(v)))}
        r["warnings"] = sorted({type(w.message).__name__ for w in rec})
        return r
    except Exception as e:  # noqa: BLE001 (the reference's own exception types are the data)
        return {"raises": type(e).__name__}


xr = x.real[:2000].copy()
conv = {
    "psd_list": outcome(lambda: ss.psd(list(xr), 256)),
    "psd_int64": outcome(lambda: ss.psd(np.arange(2000) % 17, 256)),
    "psd_2d": outcome(lambda: ss.psd(xr.reshape(2, 1000), 256)),
    "psd_K0": outcome(lambda: ss.psd(xr[:256], 256)),
    "psd_K0_complex": outcome(lambda: ss.psd(x[:100], 256)),
    "psd_empty": outcome(lambda: ss.psd(np.zeros(0), 256)),
    "my_psd_list": outcome(lambda: ss.my_psd(list(xr), 256)),
    "my_psd_int64": outcome(lambda: ss.my_psd(np.arange(2000) % 17, 256)),
    "my_psd_2d": outcome(lambda: ss.my_psd(xr.reshape(2, 1000), 256)),
    "my_psd_short": outcome(lambda: ss.my_psd(xr[:100], 256)),
    "simple_sa_list": outcome(lambda: ss.simple_sa(list(xr), 128, 512, 1)),
    "simple_sa_int64": outcome(lambda: ss.simple_sa(np.arange(2000) % 17, 128, 512, 1)),
    "simple_sa_2d": outcome(lambda: ss.simple_sa(xr.reshape(2, 1000), 128, 512, 1)),
    "simple_sa_NAVG_gt_K": outcome(lambda: ss.simple_sa(xr, 128, 512, 1, NAVG=16)),
    "simple_sa_complex64": outcome(lambda: ss.simple_sa(x[:2000].astype(np.complex64), 128, 512, 1)),
    "simple_sa_complex128": outcome(lambda: ss.simple_sa(x[:2000], 128, 512, 1)),
    "deliberate_differences": {
        "psd_overlap_100": "the reference never terminates (step = 0); here ValueError",
        "psd_2d / my_psd_2d / simple_sa_2d": "here ValueError: x must be one-dimensional",
        "simple_sa_log": "the reference's malformed log.info('K = ', K) is not reproduced",
    },
}
with open(os.path.join(HERE, "g16_conventions.json"), "w") as fh:
    json.dump(conv, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("g16: %d cases, %d bytes" % (len(cases), os.path.getsize(os.path.join(HERE, "g16_psd.npz"))))
