"""Timing of the pulse shaping and matched filter kernels over frame sets (csrc/pulse.hip) beside the routes they replace.

Workload: 4096 frames x 2048 symbols, complex64 and complex128, the src pulse of m = 6 (2 m ns + 1 taps) at ns = 4, 8, 16.

  shape     pulse_shape_rows_kernel: ms, the bytes it must move (symbols in, ns times as many samples out) as a fraction of the device-copy rate of
            the same run; beside it the parent's route on the same buffers: skdsp_upsample_dev on the flattened set, then skdsp_fir_filter_rows_dev
  mf        pulse_mf_rows_kernel at start = 2 m ns, step = ns: ms, the float64 operation rate (4 ntaps per complex output: two products and two sums
            per tap), the bytes as a fraction of the device-copy rate; beside it the parent's route, skdsp_fir_filter_rows_dev at the full rate
            (whose caller then reads z[start::ns]), and two A/B builds of the same kernel: option pulse_mf_variant = 1 (the staged window in its
            natural order: the naive LDS layout) and = 2 (each product and sum contracted into one fused multiply-add: what the bit-exact recipe costs)

    python tools/time_pulse.py [shape mf] [--reps K] [--rows R] [--json PATH]

Device data stays on the device; per measurement, device events around each of K launches after a warm-up, median of the repeats; the routes of one
comparison alternate within the same run.  One JSON line per measurement, stamped with the hashes of the kernels' sources; --json appends them to
PATH (default profiles/r17/time_pulse.json)."""
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

PARTS = ("shape", "mf")
NSYM, M_SPAN = 2048, 6


def source_hashes():
    out = {}
    for name in ("pulse.hip", "pulse_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def alternating(launches, reps):
    """median ms of each launch, the launches taken in turn so that a drift of the clock meets all of them"""
    import statistics
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


def main(argv):
    from time_blockcode import device_copy_gbps
    parts = [a for a in argv if a in PARTS] or list(PARTS)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    nrow = int(argv[argv.index("--rows") + 1]) if "--rows" in argv else 4096
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else os.path.join(ROOT, "profiles", "r17", "time_pulse.json")
    stamp = source_hashes()
    _ffi.init(0)
    device = _ffi.device_info()["name"]
    src, dst = _ffi.DeviceBytes(1 << 28), _ffi.DeviceBytes(1 << 28)
    copy = device_copy_gbps(src.ptr, dst.ptr, 1 << 28)
    src.free()
    dst.free()
    recs = []
    for dtype in (np.complex64, np.complex128):
        esz = np.dtype(dtype).itemsize
        for ns in (4, 8, 16):
            taps = ss.sqrt_rc_imp(ns, 0.35, M_SPAN)
            b = taps / np.sum(taps)
            n, start = NSYM * ns, 2 * M_SPAN * ns
            n_out = _ffi.sym_count(n, start, ns)
            sym = _ffi.DeviceArray(nrow * NSYM, dtype).fill_noise(41)
            stuffed, x, y = (_ffi.DeviceArray(nrow * n, dtype) for _ in range(3))
            z = _ffi.DeviceArray(nrow * n_out, dtype)
            base = {"dtype": np.dtype(dtype).name, "nrow": nrow, "symbols_per_row": NSYM, "ns": ns, "ntaps": int(taps.size), "device": device,
                    "device_copy_GBps": round(copy, 1), "source_sha256": stamp}
            if "shape" in parts:
                new, old = _ffi.PulseKernel(taps, dtype), _ffi.FirKernel(taps, _ffi.code_of(dtype))
                up = lambda: _ffi.check(_ffi.load().skdsp_upsample_dev(_ffi._dp(sym), nrow * NSYM, ns, _ffi.code_of(dtype), 1.0, _ffi._dp(stuffed)))
                (ms, rounds), (ms_up, r_up), (ms_fir, r_fir) = alternating(
                    [lambda: new.shape_rows_dev(sym, x, NSYM, nrow, ns), up, lambda: old.filter_rows_dev(stuffed, y, n, nrow)], reps)
                nbytes = nrow * (NSYM + n) * esz
                recs.append(dict(base, part="shape", kernel="pulse_shape_rows", ms=round(ms, 4), bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1),
                                 frac_of_device_copy=round(nbytes / ms / 1e6 / copy, 3), parent_route="upsample_dev + fir_filter_rows_dev",
                                 parent_ms=round(ms_up + ms_fir, 4), parent_upsample_ms=round(ms_up, 4), parent_fir_rows_ms=round(ms_fir, 4),
                                 new_over_parent=round(ms / (ms_up + ms_fir), 3), ms_rounds=rounds, parent_rounds=[r_up, r_fir]))
            else:
                _ffi.PulseKernel(taps, dtype).shape_rows_dev(sym, x, NSYM, nrow, ns)
            if "mf" in parts:
                new, old = _ffi.PulseKernel(b, dtype), _ffi.FirKernel(b, _ffi.code_of(dtype))

                def variant(v):
                    def run():
                        with _ffi.option("pulse_mf_variant", v):
                            new.mf_rows_dev(x, z, n, nrow, start, ns)
                    return run
                (ms, rounds), (ms_old, r_old), (ms_naive, r_naive), (ms_fma, r_fma) = alternating(
                    [variant(0), lambda: old.filter_rows_dev(x, y, n, nrow), variant(1), variant(2)], reps)
                nbytes = nrow * (n + n_out) * esz
                flops = 4.0 * taps.size * n_out * nrow
                recs.append(dict(base, part="mf", kernel="pulse_mf_rows", start=start, step=ns, ms=round(ms, 4), bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1),
                                 frac_of_device_copy=round(nbytes / ms / 1e6 / copy, 3), f64_gflop_s=round(flops / ms / 1e6, 1),
                                 parent_route="fir_filter_rows_dev at the full rate", parent_ms=round(ms_old, 4), new_over_parent=round(ms / ms_old, 3),
                                 naive_layout_ms=round(ms_naive, 4), swizzled_over_naive=round(ms / ms_naive, 3), fma_contracted_ms=round(ms_fma, 4),
                                 exact_over_fma=round(ms / ms_fma, 3), ms_rounds=rounds, parent_rounds=r_old, naive_rounds=r_naive, fma_rounds=r_fma))
            for d in (sym, stuffed, x, y, z):
                d.free()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        for r in recs:
            line = json.dumps(r, sort_keys=True)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
