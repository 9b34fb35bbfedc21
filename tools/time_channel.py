"""Timing of the channel and source kernels (csrc/channel.hip): awgn (complex64, complex128, float32; in place), the channel on bits, random
bits, the m-sequence source (m = 16) and the rows' sigma and gain, beside DeviceArray.fill_noise -- the benchmark's input filler, the
cheapest existing draw -- on the same buffers.

  rows     4096 frames x 16384 elements
  stream   one row of 2^26 elements

    python tools/time_channel.py [rows stream] [--reps K] [--json PATH]

All data stays on the device; per kernel, device events around each of K single launches after a warm-up, median of the repeats (7 by
default): ms, the bytes the kernel must read plus the bytes it writes over that time in GB/s and as a fraction of the device-copy rate
measured in the same run the way bench.py --full measures it (hipMemcpyAsync device-to-device of 2^28 bytes, bytes read + bytes written),
and elements per second.  "sigma" is the three launches of awgn_sigma_rows_dev.  Nothing is asserted on time.  One JSON line per
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

from sk_dsp_comm_amd import _ffi, sigsys as ss  # noqa: E402
from time_blockcode import device_copy_gbps, median_ms  # noqa: E402

SHAPES = {"rows": (4096, 16384), "stream": (1, 1 << 26)}
DTYPES = (np.complex64, np.complex128, np.float32)


def source_hashes():
    out = {}
    for name in ("channel.hip", "channel_core.hpp", "symmap.hip", "symmap_core.hpp", "resample.hip"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def run_shape(name, nrow, n, reps, copy, stamp):
    recs = []

    def record(kernel, dtype, launch, nbytes):
        _ffi.debug_path()
        ms, rounds = median_ms(launch, reps)
        recs.append({"shape": name, "nrow": nrow, "elements_per_row": n, "kernel": kernel, "dtype": dtype, "ms": round(ms, 4), "bytes": nbytes,
                     "GBps": round(nbytes / ms / 1e6, 1), "device_copy_GBps": round(copy, 1), "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 3),
                     "gelem_s": round(nrow * n / ms / 1e6, 2), "ms_rounds": [round(v, 4) for v in rounds], "path": sorted(set(_ffi.debug_path())),
                     "source_sha256": stamp})
        print(json.dumps(recs[-1]), flush=True)

    gd, sd = _ffi.DeviceArray(nrow, np.float64), _ffi.DeviceArray(nrow, np.float64)
    for dtype in DTYPES:
        esz = np.dtype(dtype).itemsize
        xd = _ffi.DeviceArray(nrow * n, dtype).fill_noise(14)
        record("fill_noise", np.dtype(dtype).name, lambda: xd.fill_noise(14), nrow * n * esz)
        record("sigma", np.dtype(dtype).name, lambda: _ffi.awgn_sigma_rows_dev(xd, n, nrow, _ffi.SIGMA_AWGN, 1, 10.0, gd, sd), nrow * (n * esz + 16))
        record("awgn", np.dtype(dtype).name, lambda: _ffi.awgn_rows_dev(xd, xd, n, nrow, 15, gd=gd, sd=sd), 2 * nrow * n * esz)
        xd.free()
    bits, out = _ffi.DeviceBytes(nrow * n), _ffi.DeviceBytes(nrow * n)
    record("random_bits", "uint8", lambda: _ffi.random_bits_rows_dev(bits, n, nrow, 16), nrow * n)
    record("awgn_bits", "uint8", lambda: _ffi.awgn_bits_rows_dev(bits, out, n, nrow, 17, sigma=0.5), 2 * nrow * n)
    c = ss._mseq_bytes(16)
    cd, pd = _ffi.device_bytes_of(c), _ffi.device_bytes_of((np.arange(nrow, dtype=np.int64) * 977) % c.size)
    record("pn", "uint8", lambda: _ffi.pn_rows_dev(cd, c.size, out, n, nrow, phases_d=pd), nrow * n)
    for d in (gd, sd, bits, out, cd, pd):
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
        lines += run_shape(name, SHAPES[name][0], SHAPES[name][1], reps, copy, stamp)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
