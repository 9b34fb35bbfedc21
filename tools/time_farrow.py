"""Timing of the Farrow resampler (csrc/farrow.hip) on its three workloads, 2^26 input samples, i_ord = 3, default dtypes:

  W1  complex64  48000 -> 44100  (complex128 out)
  W2  float32    8 -> 18         (float64 out)
  W3  float64    1 -> pi

    python tools/time_farrow.py [W1 W2 W3] [--reps K] [--no-numpy] [--json PATH]

Per workload: ms per pass of skdsp_farrow_dev (device events around K launches after a warm-up), algorithmic TB/s
(esz_in n + esz_out N bytes), its fraction of 8 TB/s, the engine skdsp_debug_path names, and -- as the CPU yardstick,
since the reference itself does not run where the GPU is -- the vectorised NumPy restatement of the reference's loop
(tests/test_farrow_cpu.py) timed on one core over 2^22 outputs.  One JSON line per workload."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi  # noqa: E402

WORKLOADS = {"W1": (np.complex64, 48000.0, 44100.0), "W2": (np.float32, 8.0, 18.0), "W3": (np.float64, 1.0, np.pi)}
PEAK_TBS = 8.0


def main(argv):
    names = [a for a in argv if a in WORKLOADS] or list(WORKLOADS)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 100
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    _ffi.init(0)
    n = 1 << 26
    lines = []
    for name in names:
        dt, fs_old, fs_new = WORKLOADS[name]
        ts_old, ts_new = 1 / fs_old, 1 / fs_new
        N = _ffi.farrow_len(n, ts_old, ts_new)
        out_dt = np.result_type(dt, np.float64)
        xd = _ffi.DeviceArray(n, dt).fill_noise(1)
        yd = _ffi.DeviceArray(N, out_dt)
        _ffi.debug_path()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:
            for _ in range(10):
                _ffi.farrow_dev(xd, yd, ts_old, ts_new, 3, 0.5, wide=True)
            _ffi.sync()
        path = _ffi.debug_path()
        _ffi.timer_start()
        for _ in range(reps):
            _ffi.farrow_dev(xd, yd, ts_old, ts_new, 3, 0.5, wide=True)
        ms = _ffi.timer_stop() / reps
        nbytes = np.dtype(dt).itemsize * n + out_dt.itemsize * N
        rec = {"workload": name, "dtype": np.dtype(dt).name, "fs_old": fs_old, "fs_new": fs_new, "n_in": n, "n_out": N, "i_ord": 3,
               "ms": round(ms, 5), "alg_bytes": nbytes, "tbs": round(nbytes / ms / 1e9, 3), "frac_8tbs": round(nbytes / ms / 1e9 / PEAK_TBS, 4),
               "path": path}
        if "--no-numpy" not in argv:
            from test_farrow_cpu import farrow_restated
            m = 1 << 22
            x = xd.to_host(0, int(m * ts_new / ts_old) + 8)
            t1 = time.perf_counter()
            farrow_restated(x, fs_old, fs_new, 3, 0.5, 0, m)
            s = time.perf_counter() - t1
            rec["numpy_1core_Mout_s"] = round(m / s / 1e6, 2)
            rec["numpy_1core_ms_full"] = round(s * N / m * 1e3, 1)
        xd.free()
        yd.free()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if out_path:
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
