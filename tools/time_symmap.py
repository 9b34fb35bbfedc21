"""Timing of the Gray symbol mapping kernels (csrc/symmap.hip): map, scale and demap for 16-QAM, 256-QAM and 8-PSK, complex64 and complex128
symbols, input steps 1 and 4 (the matched filter's output read as z[start::4] without a compacting pass).

  rows     4096 frames x 16384 symbols
  stream   one row of 2^26 symbols

    python tools/time_symmap.py [rows stream] [--reps K] [--json PATH]

All data stays on the device (the symbols are the library's device noise: a time does not depend on the values); per kernel, device events
around each of K launches after a warm-up, median of the repeats: ms, the bytes the kernel must read (the symbols it decides, not the
elements between them) plus the bytes it writes over that time in GB/s and as a fraction of the device-copy rate measured in the same run
the way bench.py --full measures it (hipMemcpyAsync device-to-device of 2^28 bytes, bytes read + bytes written).  "scale" is the two launches
of qam_scale_rows_dev.  Beside them, the NumPy restatements of the reference (digitalcom.qam_gray_decode_host / mpsk_gray_decode_host) on one
core for 2^20 symbols, in symbols per second.  One JSON line per measurement, stamped with the hashes of the kernels' sources."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi, digitalcom as dc  # noqa: E402
from time_blockcode import device_copy_gbps, median_ms  # noqa: E402

SHAPES = {"rows": (4096, 16384), "stream": (1, 1 << 26)}
ORDERS = [("16qam", _ffi.QAM, 16), ("256qam", _ffi.QAM, 256), ("8psk", _ffi.MPSK, 8)]
STEPS = (1, 4)
HOST_SYMBOLS = 1 << 20


def source_hashes():
    out = {}
    for name in ("symmap.hip", "symmap_core.hpp", "blockcode_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def run_shape(name, nrow, n, reps, copy, stamp):
    recs = []
    d_bits = _ffi.DeviceBytes(8 * nrow * n)
    d_bits.write(np.random.default_rng(13).integers(0, 2, 8 * nrow * n, dtype=np.uint8))
    d_out, d_r = _ffi.DeviceBytes(8 * nrow * n), _ffi.DeviceBytes(8 * nrow)
    for dtype in (np.complex64, np.complex128):
        esz = np.dtype(dtype).itemsize
        xd = _ffi.DeviceArray(nrow * n * max(STEPS), dtype).fill_noise(14)
        for label, kind, mod in ORDERS:
            bps = _ffi.sym_bits(kind, mod)
            runs = [("map", 1, "symmap", lambda: _ffi.gray_map_rows_dev(d_bits.ptr, bps * n, n, nrow, kind, mod, dtype, xd.ptr), nrow * n * (bps + esz))]
            for step in STEPS:
                if kind == _ffi.QAM:
                    runs.append(("scale", step, "symscale", lambda step=step: _ffi.qam_scale_rows_dev(xd.ptr, n * step, 0, step, n, nrow, dtype, mod, d_r.ptr), nrow * (n * esz + 8)))
                runs.append(("demap", step, "symdemap", lambda step=step: _ffi.gray_demap_rows_dev(xd.ptr, n * step, 0, step, n, nrow, dtype, kind, mod, d_out.ptr, r_ptr=d_r.ptr),
                             nrow * n * (bps + esz)))
            for kernel, step, engine, launch, nbytes in runs:
                if kernel != "map" and step == STEPS[0]:
                    xd.fill_noise(14)          # (the mapper wrote constellation points over the first rows: back to noise for every order alike)
                _ffi.debug_path()
                ms, rounds = median_ms(launch, reps)
                recs.append({"shape": name, "nrow": nrow, "symbols_per_row": n, "order": label, "dtype": np.dtype(dtype).name, "kernel": kernel, "step": step,
                             "ms": round(ms, 4), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "device_copy_GBps": round(copy, 1),
                             "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 3), "gsym_s": round(nrow * n / ms / 1e6, 2), "ms_rounds": [round(v, 4) for v in rounds],
                             "path": sorted(set(_ffi.debug_path())), "engine": engine, "source_sha256": stamp})
        xd.free()
    for d in (d_bits, d_out, d_r):
        d.free()
    return recs


def host_forms(stamp):
    """the vectorised NumPy restatements of the reference's demappers on one core (the reference itself loops over the symbols in Python)"""
    rng = np.random.default_rng(15)
    recs = []
    for label, kind, mod in ORDERS:
        bits = rng.integers(0, 2, (1, HOST_SYMBOLS * _ffi.sym_bits(kind, mod)), dtype=np.uint8)
        x = _ffi.gray_map_rows_host(bits, kind, mod)[0] + 0.05 * (rng.standard_normal(HOST_SYMBOLS) + 1j * rng.standard_normal(HOST_SYMBOLS))
        fn = dc.qam_gray_decode_host if kind == _ffi.QAM else dc.mpsk_gray_decode_host
        fn(x[:1024], mod)
        t0 = time.perf_counter()
        fn(x, mod)
        dt = time.perf_counter() - t0
        recs.append({"shape": "host", "order": label, "dtype": "complex128", "kernel": "decode_host", "symbols": HOST_SYMBOLS, "ms": round(1e3 * dt, 2),
                     "gsym_s": round(HOST_SYMBOLS / dt / 1e9, 4), "source_sha256": stamp})
    return recs


def main(argv):
    names = [a for a in argv if a in SHAPES] or list(SHAPES)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    _ffi.init(0)
    src, dst = _ffi.DeviceBytes(1 << 28), _ffi.DeviceBytes(1 << 28)
    copy = device_copy_gbps(src.ptr, dst.ptr, 1 << 28)
    src.free()
    dst.free()
    stamp = source_hashes()
    lines = []
    for name in names:
        for rec in run_shape(name, SHAPES[name][0], SHAPES[name][1], reps, copy, stamp):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    for rec in host_forms(stamp):
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
