"""Timing of the symbol-error kernels (csrc/symerr.hip).

  lagcorr   lagcorr_kernel + lagmerge_kernel at K = 2^20 and 2^24 samples, n_lags = 1024 (2049 lags), complex64 and complex128: ms and the
            achieved float64 FMA rate, 4 K lags / time
  count     symcount_kernel on 4096 frames x 16384 symbols, 16-QAM / 256-QAM / QPSK / BPSK, complex64 and complex128: ms, the bytes it must move
            (both streams + 32 bytes per row) over that time as a fraction of the device-copy rate taken in the same run
  gray      gray_demap_rows_dev + bit_count_rows_dev on the same 16-QAM symbols: the Gray route writes and re-reads a byte per bit
  host      qam_sep_host (NumPy, the reference's FFT search in exact form) on one core, 2^20 symbols of 16-QAM
  reference the reference's own qam_sep on one core at 2^18 symbols; runs WITHOUT a GPU where sk_dsp_comm can be imported
            (SK_DSP_COMM_SRC names its source directory), skipped with a note otherwise

    python tools/time_symerr.py [lagcorr count gray host reference] [--reps K] [--json PATH]

Device data stays on the device; per measurement, device events around each of K launches after a warm-up, median of the repeats.  One JSON line
per measurement, stamped with the hashes of the kernels' sources; --json appends them to PATH (default profiles/r16/time_symerr.json)."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi, digitalcom as dc  # noqa: E402

PARTS = ("lagcorr", "count", "gray", "host", "reference")
NROW, NSYM = 4096, 16384


def source_hashes():
    out = {}
    for name in ("symerr.hip", "symerr_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def qam_frames(rng, M, count):
    tx = (2 * rng.integers(0, M, count) - (M - 1)) + 1j * (2 * rng.integers(0, M, count) - (M - 1))
    return tx, tx / (M - 1) + (0.46 / (M - 1)) * (rng.standard_normal(count) + 1j * rng.standard_normal(count))


def time_lagcorr(reps, stamp):
    from time_blockcode import median_ms
    recs = []
    for log2 in (20, 24):
        K = 1 << log2
        for dtype in (np.complex64, np.complex128):
            a, b = _ffi.DeviceArray(K, dtype).fill_noise(31), _ffi.DeviceArray(K, dtype).fill_noise(32)
            nl, _ = _ffi.lag_corr_len(K, 1024)
            out = _ffi.DeviceArray(nl + 1, np.complex128)
            ms, rounds = median_ms(lambda: _ffi.lag_corr_dev(a, b, K, 1024, out.ptr, out.ptr + 16 * nl), reps)
            recs.append({"part": "lagcorr", "K": K, "lags": nl, "dtype": np.dtype(dtype).name, "ms": round(ms, 4), "f64_gfma_s": round(4.0 * K * nl / ms / 1e6, 1),
                         "ms_rounds": [round(v, 4) for v in rounds], "source_sha256": stamp})
            for d in (a, b, out):
                d.free()
    return recs


def time_count(reps, stamp, with_gray):
    from time_blockcode import device_copy_gbps, median_ms
    rng = np.random.default_rng(33)
    recs = []
    n = NROW * NSYM
    src, dst = _ffi.DeviceBytes(1 << 28), _ffi.DeviceBytes(1 << 28)
    copy = device_copy_gbps(src.ptr, dst.ptr, 1 << 28)
    src.free()
    dst.free()
    cnt = _ffi.DeviceBytes(32 * NROW)
    tx, rx = qam_frames(rng, 4, n)             # noisy 16-QAM for every order: a time does not depend on the values, the preconditions hold for all
    for dtype in (np.complex64, np.complex128):
        esz = np.dtype(dtype).itemsize
        txd, rxd = _ffi.DeviceArray.from_host(tx.astype(dtype)), _ffi.DeviceArray.from_host(rx.astype(dtype))
        for label, mode, M in (("16qam", _ffi.SYM_QAM, 4), ("256qam", _ffi.SYM_QAM, 16), ("qpsk", _ffi.SYM_QPSK, 0), ("bpsk", _ffi.SYM_BPSK, 0)):
            launch = lambda: _ffi.sym_count_rows_dev(txd, dtype, NSYM, 0, rxd, dtype, NSYM, 0, 1, 0, NSYM, NROW, mode, M, 1, cnt)
            ms, rounds = median_ms(launch, reps)
            nbytes = 2 * n * esz + 32 * NROW
            rec = {"part": "count", "kernel": "symcount", "order": label, "dtype": np.dtype(dtype).name, "nrow": NROW, "symbols_per_row": NSYM, "ms": round(ms, 4),
                   "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "device_copy_GBps": round(copy, 1), "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 3),
                   "ms_rounds": [round(v, 4) for v in rounds], "source_sha256": stamp}
            recs.append(rec)
            if with_gray and label == "16qam":
                # the Gray route on the same symbols: decisions to a byte per bit, then the byte count against the sent bits
                bits, dec, r = _ffi.DeviceBytes(4 * n), _ffi.DeviceBytes(4 * n), _ffi.DeviceBytes(8 * NROW)
                bits.write(rng.integers(0, 2, 4 * n, dtype=np.uint8))
                bcnt = _ffi.DeviceBytes(8 * NROW)
                _ffi.qam_scale_rows_dev(rxd.ptr, NSYM, 0, 1, NSYM, NROW, dtype, 16, r.ptr)

                def gray():
                    _ffi.gray_demap_rows_dev(rxd.ptr, NSYM, 0, 1, NSYM, NROW, dtype, _ffi.QAM, 16, dec.ptr, r_ptr=r.ptr)
                    _ffi.bit_count_rows_dev(bits.ptr, 4 * NSYM, dec.ptr, 4 * NSYM, 4 * NSYM, NROW, False, bcnt.ptr)
                gms, grounds = median_ms(gray, reps)
                gbytes = n * esz + 4 * n + 2 * 4 * n + 16 * NROW
                recs.append({"part": "gray", "kernel": "symdemap + bitcount", "order": label, "dtype": np.dtype(dtype).name, "nrow": NROW, "symbols_per_row": NSYM,
                             "ms": round(gms, 4), "bytes": gbytes, "fused_ms": round(ms, 4), "fused_bytes": nbytes, "fused_over_gray": round(ms / gms, 3),
                             "ms_rounds": [round(v, 4) for v in grounds], "source_sha256": stamp})
                for d in (bits, dec, r, bcnt):
                    d.free()
        txd.free()
        rxd.free()
    cnt.free()
    return recs


def time_host(stamp):
    rng = np.random.default_rng(34)
    tx, rx = qam_frames(rng, 4, 1 << 20)
    rx = np.concatenate((rx[:5], rx))
    t0 = time.perf_counter()
    res = dc.qam_sep_host(tx, rx, '16qam', SEP_disp=False)
    dt = time.perf_counter() - t0
    return [{"part": "host", "what": "qam_sep_host (NumPy, one core)", "symbols": int(res[0]), "errors": int(res[1]), "s": round(dt, 3), "msym_s": round(res[0] / dt / 1e6, 2),
             "source_sha256": stamp}]


def time_reference(stamp):
    sys.path.insert(0, os.environ.get("SK_DSP_COMM_SRC", ""))
    try:
        os.environ.setdefault("MPLBACKEND", "Agg")
        from sk_dsp_comm import digitalcom as ref
    except Exception as e:
        return [{"part": "reference", "skipped": "sk_dsp_comm cannot be imported here (%s)" % type(e).__name__}]
    rng = np.random.default_rng(35)
    tx, rx = qam_frames(rng, 4, 1 << 18)
    rx = np.concatenate((rx[:5], rx))
    t0 = time.perf_counter()
    res = ref.qam_sep(tx, rx, '16qam', SEP_disp=False)
    dt = time.perf_counter() - t0
    return [{"part": "reference", "what": "sk_dsp_comm.digitalcom.qam_sep (one core)", "symbols": int(res[0]), "errors": int(res[1]), "s": round(dt, 3),
             "msym_s": round(res[0] / dt / 1e6, 3), "numpy": np.__version__, "source_sha256": stamp}]


def main(argv):
    parts = [a for a in argv if a in PARTS] or ["lagcorr", "count", "gray", "host"]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else os.path.join(ROOT, "profiles", "r16", "time_symerr.json")
    stamp = source_hashes()
    recs = []
    if {"lagcorr", "count", "gray"} & set(parts):
        _ffi.init(0)
        device = _ffi.device_info()["name"]
        if "lagcorr" in parts:
            recs += time_lagcorr(reps, stamp)
        if "count" in parts or "gray" in parts:
            got = time_count(reps, stamp, "gray" in parts)
            recs += [r for r in got if r["part"] in parts]
        for r in recs:
            r["device"] = device
    if "host" in parts:
        recs += time_host(stamp)
    if "reference" in parts:
        recs += time_reference(stamp)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        for r in recs:
            line = json.dumps(r, sort_keys=True)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
