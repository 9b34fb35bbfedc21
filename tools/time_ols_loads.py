"""Time the overlap-save kernels that share load_tile (csrc/fir_ols.hip) under the values of the option ols_keep_overlap, as bench.py makes the workloads
(1024 taps, complex64, 2^26 samples at the high rate): fir1024 (.filter), firdn4 (.dn(x, 4)), firup4 (.up(x, 4)); with --only also fir1024f32 (.filter, float32).
    python tools/time_ols_loads.py [--reps 1] [--only fir1024,firdn4] v1 v2 ...
One line per (workload, value, rep); SKDSP_LIB selects another build of the library, so that a shell loop can alternate two builds on one box."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
import numpy as np
import bench
from sk_dsp_comm_amd import _ffi
args = sys.argv[1:]
reps, only = 1, ("fir1024", "firdn4", "firup4")
if "--reps" in args:
    i = args.index("--reps"); reps = int(args[i + 1]); del args[i:i + 2]
if "--only" in args:
    i = args.index("--only"); only = tuple(args[i + 1].split(",")); del args[i:i + 2]
vals = [int(v) for v in args] or [_ffi.get_option("ols_keep_overlap")]
n = 1 << 26
_ffi.init(0)
lib = os.path.basename(os.environ.get("SKDSP_LIB", "default"))
work = {}
if "fir1024" in only:
    k = _ffi.FirKernel(bench.firwin_lowpass(1024, 0.2), _ffi.C64)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=1024).fill_noise(1); yd = _ffi.DeviceArray(n, np.complex64)
    work["fir1024"] = (lambda k=k, xd=xd, yd=yd: k.filter_dev(xd, yd))
if "fir1024f32" in only:
    kf = _ffi.FirKernel(bench.firwin_lowpass(1024, 0.2), _ffi.F32)
    xf = _ffi.DeviceArray(n, np.float32, headroom=1024).fill_noise(1); yf = _ffi.DeviceArray(n, np.float32)
    work["fir1024f32"] = (lambda: kf.filter_dev(xf, yf))
if "firdn4" in only:
    k4 = _ffi.FirKernel(bench.firwin_lowpass(1024, 0.2 / 4), _ffi.C64)
    xd4 = _ffi.DeviceArray(n, np.complex64, headroom=1024).fill_noise(1); yd4 = _ffi.DeviceArray(n // 4, np.complex64)
    work["firdn4"] = (lambda: k4.dn_dev(xd4, yd4, 4))
if "firup4" in only:
    ku = _ffi.FirKernel(bench.firwin_lowpass(1024, 0.2 / 4), _ffi.C64)
    xu = _ffi.DeviceArray(n // 4, np.complex64, headroom=1024).fill_noise(1); yu = _ffi.DeviceArray(n, np.complex64)
    work["firup4"] = (lambda: ku.up_dev(xu, yu, 4))
def settle(fn, seconds=0.5):   # (the clock leaves its idle state)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50): fn()
        _ffi.sync()
def timed(fn, steps=300):
    for _ in range(100): fn()
    _ffi.sync(); _ffi.timer_start()
    for _ in range(steps): fn()
    return _ffi.timer_stop() / steps
for name, fn in work.items():
    settle(fn)
    for rep in range(reps):
        for v in vals:
            _ffi.set_option("ols_keep_overlap", v)
            _ffi.debug_path()
            ms = timed(fn)
            print("%s %s ols_keep_overlap=%d: %.4f ms  (%s)" % (lib, name, v, ms, ",".join(sorted(set(_ffi.debug_path())))), flush=True)
