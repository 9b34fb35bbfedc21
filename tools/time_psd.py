"""Timing of the Welch primitive (csrc/psd.hip): 2^26 samples, Hann window, 50 % overlap (K = 2^27 / n_fft - 2 segments as
sigsys.psd counts them):

  C256 C1024 C4096   complex64, n_fft = 256 / 1024 / 4096
  F1024              float32,   n_fft = 1024
  D1024              float64,   n_fft = 1024

    python tools/time_psd.py [C256 C1024 C4096 F1024 D1024] [--reps K] [--no-numpy] [--json PATH]

Per workload: ms per pass of skdsp_psd_dev (device events around K launches after a warm-up; a pass is the segment kernel
plus the row reduction), algorithmic TB/s (input bytes only: the result is n_fft numbers), its fraction of 8 TB/s, the engine
skdsp_debug_path names, and -- as the CPU yardstick, since the reference itself does not run where the GPU is -- the host
float64 restatement (sigsys.psd_accum_host) timed on one core over 2^22 samples.  One JSON line per workload."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))

import numpy as np  # noqa: E402
from scipy.signal import windows  # noqa: E402

from sk_dsp_comm_amd import _ffi, sigsys as ss  # noqa: E402

WORKLOADS = {"C256": (np.complex64, 256), "C1024": (np.complex64, 1024), "C4096": (np.complex64, 4096),
             "F1024": (np.float32, 1024), "D1024": (np.float64, 1024)}
PEAK_TBS = 8.0


def main(argv):
    names = [a for a in argv if a in WORKLOADS] or list(WORKLOADS)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 100
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    _ffi.init(0)
    n = 1 << 26
    lines = []
    for name in names:
        dt, n_fft = WORKLOADS[name]
        step, K = ss._psd_segments(n, n_fft, 50)
        w = windows.hann(n_fft)
        xd = _ffi.DeviceArray(n, dt).fill_noise(1)
        Sd = _ffi.DeviceArray(n_fft, np.float64)
        _ffi.debug_path()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:
            for _ in range(10):
                _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, K)
            _ffi.sync()
        path = _ffi.debug_path()
        _ffi.timer_start()
        for _ in range(reps):
            _ffi.psd_accum_dev(xd, Sd, w, n_fft, step, K)
        ms = _ffi.timer_stop() / reps
        nbytes = np.dtype(dt).itemsize * n
        rec = {"workload": name, "dtype": np.dtype(dt).name, "n": n, "n_fft": n_fft, "step": step, "segments": K, "ms": round(ms, 5),
               "alg_bytes": nbytes, "tbs": round(nbytes / ms / 1e9, 3), "frac_8tbs": round(nbytes / ms / 1e9 / PEAK_TBS, 4), "path": path}
        if "--no-numpy" not in argv:
            m = 1 << 22
            x = xd.to_host(0, m)
            km = ss._psd_segments(m, n_fft, 50)[1]
            t1 = time.perf_counter()
            ref = ss.psd_accum_host(x, w, n_fft, step, km)
            s = time.perf_counter() - t1
            rec["numpy_1core_Msamples_s"] = round(m / s / 1e6, 2)
            rec["numpy_1core_ms_full"] = round(s * n / m * 1e3, 1)
            Sm = _ffi.DeviceArray(n_fft, np.float64)
            _ffi.psd_accum_dev(xd, Sm, w, n_fft, step, km)
            rec["peak_rel_err_2p22"] = float(np.max(np.abs(Sm.to_host() - ref)) / ref.max())
            Sm.free()
        xd.free()
        Sd.free()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if out_path:
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
