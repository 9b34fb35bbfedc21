"""Timing of the OFDM kernels (csrc/ofdm.hip): ofdm_tx and ofdm_rx (nf = nc / 2, a cyclic prefix of nc / 8, no pilots) at nc = 64, 1024, 4096
in complex64 and complex128, beside psd_kernel -- the existing kernel on the same in-LDS transform -- at the same n_fft and dtype over the same
samples (rectangular window, no overlap), and the device-copy rate of the same run.

  rows     4096 frames x 256 symbols; fewer frames where they would exceed 2^26 samples (nc = 1024: 256 frames, nc = 4096: 64)
  stream   one row of 2^26 / nc symbols

    python tools/time_ofdm.py [rows stream] [--reps K] [--json PATH]

All data stays on the device; per kernel, device events around each of K single launches after a warm-up, median of the repeats (7 by
default): ms, the bytes the kernel must read plus the bytes it writes over that time in GB/s and as a fraction of the device-copy rate
measured in the same run the way bench.py --full measures it, and OFDM symbols per second.  Nothing is asserted on time.  One JSON line per
measurement, stamped with the hashes of the kernels' sources."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi  # noqa: E402
from time_blockcode import device_copy_gbps, median_ms  # noqa: E402

SHAPES = ("rows", "stream")
NCS = (64, 1024, 4096)
DTYPES = (np.complex64, np.complex128)
BUDGET = 1 << 26   # samples per launch


def shape_of(name, nc):
    if name == "rows":
        return min(4096, BUDGET // (256 * nc)), 256
    return 1, BUDGET // nc


def source_hashes():
    out = {}
    for name in ("ofdm.hip", "ofdm_core.hpp", "psd.hip", "psd_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def run_shape(name, nc, reps, copy, stamp):
    recs = []
    nrow, nsym = shape_of(name, nc)
    nf, ncp = nc // 2, nc // 8

    def record(kernel, dtype, launch, nbytes):
        _ffi.debug_path()
        ms, rounds = median_ms(launch, reps)
        recs.append({"shape": name, "nc": nc, "nf": nf, "ncp": ncp, "nrow": nrow, "symbols_per_row": nsym, "kernel": kernel, "dtype": dtype, "ms": round(ms, 4),
                     "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "device_copy_GBps": round(copy, 1), "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 3),
                     "msym_s": round(nrow * nsym / ms / 1e3, 2), "ms_rounds": [round(v, 4) for v in rounds], "path": sorted(set(_ffi.debug_path())),
                     "source_sha256": stamp})
        print(json.dumps(recs[-1]), flush=True)

    window = np.ones(nc)
    for dtype in DTYPES:
        esz = np.dtype(dtype).itemsize
        n_q, n_t = nrow * nsym * nf, nrow * nsym * (nc + ncp)
        qd, td, Sd = _ffi.DeviceArray(n_q, dtype).fill_noise(24), _ffi.DeviceArray(n_t, dtype).fill_noise(25), _ffi.DeviceArray(nc, np.float64)
        record("ofdm_tx", np.dtype(dtype).name, lambda: _ffi.ofdm_tx_rows_dev(qd, td, nsym, nrow, nf, nc, 0, True, ncp), (n_q + n_t) * esz)
        record("ofdm_rx", np.dtype(dtype).name, lambda: _ffi.ofdm_rx_rows_dev(td, qd, nsym, nrow, nf, nc, 0, True, ncp), (n_q + n_t) * esz)
        record("psd", np.dtype(dtype).name, lambda: _ffi.psd_accum_dev(td, Sd, window, nc, nc, nrow * nsym), nrow * nsym * nc * esz)
        for d in (qd, td, Sd):
            d.free()
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
        for nc in NCS:
            lines += run_shape(name, nc, reps, copy, stamp)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
