"""Timing of the Viterbi decoder (csrc/viterbi.hip), rate 1/2:

  S3 S5 S7 S9   soft (int16 values, quant_level 3), K = 3 / 5 / 7 / 9, decision depth 10 / 25 / 35 / 45
  U7            unquant (float64 values), K = 7, decision depth 35

    python tools/time_viterbi.py [S3 S5 S7 S9 U7] [--reps K] [--json PATH]

Per workload, device events around K launches after a warm-up, median of the repeats:
  single   one stream of 2^20 symbols through skdsp_viterbi_decode_dev (the stateful call: one wave): decoded Mbit/s and the
           step cost in ns per trellis step -- the number a later optimisation is measured against
  rows     4096 rows of 16384 symbols through skdsp_viterbi_decode_rows_dev (one launch): aggregate decoded Mbit/s
and beside them the reference's own rate for that K as recorded in tests/golden/g19_conventions.json (one CPU core, 300-bit
frames).  The values are uniform noise: the decoder's work per step does not depend on them.  One JSON line per workload,
stamped with the hashes of the kernel's sources."""
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi  # noqa: E402

HALF = {3: ('111', '101'), 5: ('11101', '10011'), 7: ('1111001', '1011011'), 9: ('111101011', '101110001')}
DEPTH = {3: 10, 5: 25, 7: 35, 9: 45}
WORKLOADS = {"S3": (3, 1), "S5": (5, 1), "S7": (7, 1), "S9": (9, 1), "U7": (7, 2)}
SINGLE_SYMBOLS, ROWS, ROW_SYMBOLS = 1 << 20, 4096, 16384


def source_hashes():
    out = {}
    for name in ("viterbi.hip", "viterbi_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


class Dev:
    """raw device bytes (the decoder's int16 / uint8 buffers are no sample dtype of _ffi.DeviceArray)"""

    def __init__(self, nbytes, host=None):
        p = ctypes.c_void_p(0)
        _ffi.check(_ffi.load().skdsp_malloc(ctypes.byref(p), int(nbytes) + 256))
        self.ptr = p.value
        if host is not None:
            _ffi.check(_ffi.load().skdsp_memcpy_h2d(ctypes.c_void_p(self.ptr), ctypes.c_void_p(host.ctypes.data), host.nbytes))

    def free(self):
        _ffi.check(_ffi.load().skdsp_free(ctypes.c_void_p(self.ptr)))


def median_ms(launch, reps):
    launch()
    _ffi.sync()
    ms = []
    for _ in range(reps):
        _ffi.timer_start()
        launch()
        ms.append(_ffi.timer_stop())
    return statistics.median(ms), ms


def main(argv):
    names = [a for a in argv if a in WORKLOADS] or list(WORKLOADS)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    with open(os.path.join(ROOT, "tests", "golden", "g19_conventions.json")) as f:
        ref_rate = json.load(f)["ref_bits_per_s"]
    _ffi.init(0)
    rng = np.random.default_rng(10)
    stamp = source_hashes()
    lines = []
    for name in names:
        K, metric = WORKLOADS[name]
        D = DEPTH[K]
        k = _ffi.ViterbiKernel(HALF[K], D)
        nval = 2 * ROW_SYMBOLS
        host = rng.integers(0, 8, ROWS * nval).astype(np.int16) if metric == 1 else rng.uniform(-0.5, 1.5, ROWS * nval)
        xd = Dev(host.nbytes, host)     # the single stream reads the first 2^21 values of the same buffer
        yd = Dev(max(ROWS * k.out_len(nval), k.out_len(2 * SINGLE_SYMBOLS)))
        _ffi.debug_path()
        ms_single, r_single = median_ms(lambda: k.decode_dev(xd.ptr, 2 * SINGLE_SYMBOLS, metric, 3, yd.ptr), reps)
        ms_rows, r_rows = median_ms(lambda: k.decode_rows_dev(xd.ptr, nval, ROWS, metric, 3, yd.ptr), reps)
        path = sorted(set(_ffi.debug_path()))
        bits_single, bits_rows = k.out_len(2 * SINGLE_SYMBOLS), ROWS * k.out_len(nval)
        rec = {"workload": name, "K": K, "rate": "1/2", "metric": "soft" if metric == 1 else "unquant", "depth": D,
               "single_symbols": SINGLE_SYMBOLS, "ms_single": round(ms_single, 4), "mbit_s_single": round(bits_single / ms_single / 1e3, 3),
               "ns_per_step_single": round(ms_single * 1e6 / SINGLE_SYMBOLS, 2),
               "rows": ROWS, "row_symbols": ROW_SYMBOLS, "ms_rows": round(ms_rows, 4), "mbit_s_rows": round(bits_rows / ms_rows / 1e3, 1),
               "rows_over_single": round((bits_rows / ms_rows) / (bits_single / ms_single), 1),
               "ref_bits_per_s": ref_rate[str(K)], "rows_over_reference": round(bits_rows / ms_rows * 1e3 / ref_rate[str(K)], 0),
               "ms_single_rounds": [round(v, 4) for v in r_single], "ms_rows_rounds": [round(v, 4) for v in r_rows],
               "path": path, "source_sha256": stamp}
        xd.free()
        yd.free()
        del k
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if out_path:
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
