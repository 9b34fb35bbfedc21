"""Timing of the carrier phase tracking kernel over frame sets (csrc/carrier.hip) beside the reference's Python loop.

Workload: 16384 symbols per frame, 4096 and 65536 frames, complex64 and complex128; QPSK type 0, 8-PSK type 0 and 16-QAM type 2; z_prime alone (what a
BER loop needs) and all four outputs.

  per measurement   ms per launch, symbols per second, ns per symbol per lane (the serial chain: a lane walks its row, so this is launch time over the
                    symbols of ONE row while every SIMD holds its share of waves), the bytes the launch must move (samples in, selected outputs out) as a
                    fraction of the device-copy rate of the same run, board power and shader clock read right behind the repeats
  reference         DD_carrier_sync of the reference on one core, symbols per second (where sk_dsp_comm is importable: SK_DSP_COMM_SRC names its src/;
                    --reference-only measures just that, on a machine without a GPU)

    python tools/time_carrier.py [--reps K] [--rows R ...] [--json PATH] [--reference-only]

Device data stays on the device; per row of the table, device events around each of K launches after a warm-up, median of the repeats; the launches of
one row (z_prime alone, all four outputs) alternate within the same run.  One JSON line per measurement, stamped with the hashes of the kernel's
sources; --json appends them to PATH (default profiles/r18/time_carrier.json)."""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi  # noqa: E402

NSYM = 16384
CONFIGS = (("QPSK type 0", _ffi.MPSK, 4, 0), ("8-PSK type 0", _ffi.MPSK, 8, 0), ("16-QAM type 2", _ffi.QAM, 16, 2))


def source_hashes():
    out = {}
    for name in ("carrier.hip", "carrier_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def alternating(launches, reps):
    """median ms of each launch, the launches taken in turn so that a drift of the clock meets all of them"""
    for fn in launches:
        fn()
    _ffi.sync()
    ms = [[] for _ in launches]
    for _ in range(reps):
        for i, fn in enumerate(launches):
            _ffi.timer_start()
            fn()
            ms[i].append(_ffi.timer_stop())
    return [(statistics.median(v), [round(t, 4) for t in v]) for v in ms]


def reference_rate(n=20000):
    """symbols per second of the reference's own loop on one core, per configuration; None where it cannot be imported"""
    src = os.environ.get("SK_DSP_COMM_SRC")
    if src:
        sys.path.insert(0, src)
    try:
        os.environ.setdefault("MPLBACKEND", "Agg")
        from sk_dsp_comm import synchronization as ref
    except Exception:
        return None
    if not hasattr(np, "int"):
        np.int = int          # (the reference's MPSK > 4 branch needs it: tests/golden/g27_conventions.json)
    rng = np.random.default_rng(18)
    out = {}
    for label, fam, M, det in CONFIGS:
        z = np.exp(1j * (np.pi / 4 + 0.2)) * (1 + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
        t0 = time.perf_counter()
        ref.DD_carrier_sync(z, M, 0.05, 0.707, 'MQAM' if fam == _ffi.QAM else 'MPSK', det)
        out[label] = round(n / (time.perf_counter() - t0))
    return out


def main(argv):
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else os.path.join(ROOT, "profiles", "r18", "time_carrier.json")
    recs = []
    ref = reference_rate()
    if "--reference-only" in argv:
        recs.append({"part": "reference", "what": "sk_dsp_comm.synchronization.DD_carrier_sync on one core, 20000 symbols", "symbols_per_s": ref, "numpy": np.__version__})
    else:
        from bench import _smi_sample
        from time_blockcode import device_copy_gbps
        reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
        rows = [int(v) for v in argv[argv.index("--rows") + 1].split(",")] if "--rows" in argv else [4096, 65536]
        stamp = source_hashes()
        _ffi.init(0)
        device = _ffi.device_info()["name"]
        src, dst = _ffi.DeviceBytes(1 << 28), _ffi.DeviceBytes(1 << 28)
        copy = device_copy_gbps(src.ptr, dst.ptr, 1 << 28)
        src.free()
        dst.free()
        k1, k2 = _ffi.carrier_gains(0.05, 0.707)
        for nrow in rows:
            for dtype in (np.complex64, np.complex128):
                esz = np.dtype(dtype).itemsize
                x = _ffi.DeviceArray(nrow * NSYM, dtype).fill_noise(18)
                z, a = _ffi.DeviceArray(nrow * NSYM, dtype), _ffi.DeviceArray(nrow * NSYM, dtype)
                e, t = _ffi.DeviceArray(nrow * NSYM, np.float64), _ffi.DeviceArray(nrow * NSYM, np.float64)
                rd = _ffi.DeviceArray(nrow, np.float64)
                for label, fam, M, det in CONFIGS:
                    if fam == _ffi.QAM:
                        _ffi.qam_scale_rows_dev(x.ptr, NSYM, 0, 1, NSYM, nrow, dtype, M, rd.ptr)
                    only = lambda: _ffi.dd_carrier_rows_dev(x, NSYM, nrow, fam, M, det, False, k1, k2, zd=z, rd=rd)
                    full = lambda: _ffi.dd_carrier_rows_dev(x, NSYM, nrow, fam, M, det, False, k1, k2, zd=z, ad=a, ed=e, td=t, rd=rd)
                    got = alternating([only, full], reps)
                    power, cap, sclk = _smi_sample()
                    for outputs, per_sym, (ms, rounds) in (("z_prime", 2 * esz, got[0]), ("z_prime a_hat e_phi theta_h", 3 * esz + 16, got[1])):
                        nbytes = nrow * NSYM * per_sym
                        recs.append({"part": "device", "config": label, "dtype": np.dtype(dtype).name, "nrow": nrow, "symbols_per_row": NSYM, "outputs": outputs,
                                     "ms": round(ms, 4), "symbols_per_s": round(nrow * NSYM / ms * 1e3), "ns_per_symbol_per_lane": round(ms * 1e6 / NSYM, 2),
                                     "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 4),
                                     "device_copy_GBps": round(copy, 1), "device": device, "power_w": power, "power_cap_w": cap, "sclk_mhz": sclk,
                                     "reference_symbols_per_s": None if ref is None else ref[label], "ms_rounds": rounds, "source_sha256": stamp})
                for d in (x, z, a, e, t, rd):
                    d.free()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        for r in recs:
            line = json.dumps(r, sort_keys=True)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
