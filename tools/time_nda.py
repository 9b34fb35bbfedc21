"""Timing of the symbol timing recovery kernels over frame sets (csrc/timing.hip) beside the reference's Python loop.

Workload: 16384 samples per frame at Ns = 4 (about 4093 symbols), L = 2, 4096 and 65536 frames, complex64 and complex128, every interpolator order;
QPSK through a two-symbol triangular pulse with a timing phase per row and a little noise, so that every row pulls in and tracks (the kernel only has
to be fast for rows near lock).  256 different rows are made on the host and repeated down the frame set.

  per measurement   ms per launch of the raw call (nda_rows_kernel alone: zz, e_tau, counts) and of the normalised call (plus nda_norm_kernel), symbols
                    per second, ns per symbol per lane (the serial chain: a lane walks its row, so this is launch time over the symbols of ONE row while
                    every SIMD holds its share of waves), the bytes the launch must move (samples in, symbols and timing errors out) as a fraction of the
                    device-copy rate of the same run, board power and shader clock read right behind the repeats
  reference         NDA_symb_sync of the reference on one core, symbols per second (where sk_dsp_comm is importable: SK_DSP_COMM_SRC names its src/;
                    --reference-only measures just that, on a machine without a GPU)

    python tools/time_nda.py [--reps K] [--rows R ...] [--json PATH] [--reference-only]

Device data stays on the device; device events around each of K launches after a warm-up, median of the repeats; the launches of one row of the table
(raw, normalised) alternate within the same run.  One JSON line per measurement, stamped with the hashes of the kernel's sources; --json appends them to
PATH (default profiles/r19/time_nda.json)."""
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

NSAMP, NS, L, BNTS, BLOCK = 16384, 4, 2, 0.01, 256


def source_hashes():
    out = {}
    for name in ("timing.hip", "timing_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def frames(rng, nrow, n, dtype):
    nsym = n // NS + 3
    s = (2 * rng.integers(0, 2, (nrow, nsym)) - 1) + 1j * (2 * rng.integers(0, 2, (nrow, nsym)) - 1)
    t = (np.arange(n)[None, :] + rng.uniform(0, NS, (nrow, 1))) / NS
    k = t.astype(int)
    x = np.take_along_axis(s, k, 1) * (1 - (t - k)) + np.take_along_axis(s, k + 1, 1) * (t - k)
    return (x + 0.05 * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))).astype(dtype)


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
    """symbols per second of the reference's own loop on one core, per interpolator order; None where it cannot be imported"""
    src = os.environ.get("SK_DSP_COMM_SRC")
    if src:
        sys.path.insert(0, src)
    try:
        os.environ.setdefault("MPLBACKEND", "Agg")
        from sk_dsp_comm import synchronization as ref
    except Exception:
        return None
    z = frames(np.random.default_rng(19), 1, n, np.complex128)[0]
    out = {}
    for i_ord in (1, 2, 3):
        t0 = time.perf_counter()
        zz, _ = ref.NDA_symb_sync(z, NS, L, BNTS, 0.707, i_ord)
        out[str(i_ord)] = round(zz.size / (time.perf_counter() - t0))
    return out


def main(argv):
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else os.path.join(ROOT, "profiles", "r19", "time_nda.json")
    recs = []
    ref = reference_rate()
    if "--reference-only" in argv:
        recs.append({"part": "reference", "what": "sk_dsp_comm.synchronization.NDA_symb_sync on one core, 20000 samples at Ns = 4, L = 2", "symbols_per_s": ref,
                     "numpy": np.__version__})
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
        k1, k2 = _ffi.nda_gains(BNTS, 0.707, NS)
        cap = NSAMP // NS + 64
        for nrow in rows:
            for dtype in (np.complex64, np.complex128):
                esz = np.dtype(dtype).itemsize
                block = frames(np.random.default_rng(19), min(BLOCK, nrow), NSAMP, dtype).reshape(-1)
                x = _ffi.DeviceArray(nrow * NSAMP, dtype)
                for at in range(0, nrow * NSAMP, block.size):
                    x.write(block, at)
                z, e = _ffi.DeviceArray(nrow * cap, dtype), _ffi.DeviceArray(nrow * cap, np.float64)
                cd = _ffi.device_bytes_of(np.zeros(nrow, dtype=np.int64))
                for i_ord in (1, 2, 3):
                    raw = lambda: _ffi.nda_rows_dev(x, NSAMP, nrow, NS, L, i_ord, k1, k2, cap, cd, zd=z, ed=e, normalize=False)
                    norm = lambda: _ffi.nda_rows_dev(x, NSAMP, nrow, NS, L, i_ord, k1, k2, cap, cd, zd=z, ed=e, normalize=True)
                    got = alternating([raw, norm], reps)
                    power, pcap, sclk = _smi_sample()
                    counts = cd.read().view(np.int64)
                    nsym = int(counts.sum())
                    for call, (ms, rounds) in (("raw", got[0]), ("normalised", got[1])):
                        nbytes = nrow * NSAMP * esz + nsym * (esz + 8) + (2 * nsym * (16 if esz == 8 else esz) if call == "normalised" else 0)
                        recs.append({"part": "device", "I_ord": i_ord, "Ns": NS, "L": L, "dtype": np.dtype(dtype).name, "nrow": nrow, "samples_per_row": NSAMP, "call": call,
                                     "symbols_per_row": [int(counts.min()), int(counts.max())], "ms": round(ms, 4), "symbols_per_s": round(nsym / ms * 1e3),
                                     "ns_per_symbol_per_lane": round(ms * 1e6 / (nsym / nrow), 2), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1),
                                     "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 4), "device_copy_GBps": round(copy, 1), "device": device, "power_w": power,
                                     "power_cap_w": pcap, "sclk_mhz": sclk, "reference_symbols_per_s": None if ref is None else ref[str(i_ord)], "ms_rounds": rounds,
                                     "source_sha256": stamp})
                for d in (x, z, e, cd):
                    d.free()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        for r in recs:
            line = json.dumps(r, sort_keys=True)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
