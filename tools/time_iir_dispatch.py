"""Host cost of one short IIR device call (the dispatch decision and the launch): python tools/time_iir_dispatch.py [calls] [runs]
n = 4096, the 8-biquad elliptic band-pass, float32 and complex64, filter_dev back to back, one sync at the end; microseconds per call."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
import numpy as np
from sk_dsp_comm_amd import _ffi
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 4096
sos = np.load(os.path.join(ROOT, "tests", "golden", "g7_iir_sos.npz"))["sos8"]
_ffi.init(0)
for code, npdt in ((_ffi.F32, np.float32), (_ffi.C64, np.complex64)):
    xd = _ffi.DeviceArray(n, npdt).fill_noise(7)
    yd = _ffi.DeviceArray(n, npdt)
    k = _ffi.IirKernel(code, sos=sos)
    for _ in range(200): k.filter_dev(xd, yd)
    _ffi.sync()
    us = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(calls): k.filter_dev(xd, yd)
        _ffi.sync()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    print("%s %s: us per call %s  median %.2f  spread %.2f" % (os.path.basename(os.environ.get("SKDSP_LIB", "default")), np.dtype(npdt).name,
          " ".join("%.2f" % v for v in us), float(np.median(us)), max(us) - min(us)), flush=True)
