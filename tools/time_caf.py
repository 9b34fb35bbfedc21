"""Timing of the fused FIR bank (csrc/fir_bank.hip) behind sigsys.fft_caf against the walk it replaces, one FIR pass per slice
(FirKernel.filter_dev per row: the only way to do this before the bank existed), in the same process on the same
device-resident input: 2^22 samples, a 257-sample reference, n_fft2 = 1024, slice step 1 bin:

  C9 C33 C161   complex64 signal, 9 / 33 / 161 slices
  F33           float32 signal, 33 slices (the walk has no real-input form: it runs on a complex64 copy, as fft_caf's per-band route does)

    python tools/time_caf.py [C9 C33 C161 F33] [--rounds R] [--per K] [--json PATH]

Per workload: ms per pass of both (device events; R rounds of K launches each, the two alternating, the median round; R K >= 20
after a warm-up), algorithmic TB/s against 8 n (1 + B) bytes, its fraction of 8 TB/s and of the device-copy rate measured here
(a 1 GiB device-to-device copy, read + written bytes), the ratio walk / bank, the bank with all bands in ONE group (option
fir_bank_per: the A/B of the grouping rule), the host time to create the handles and run their
first pass (the per-slice plans are built on first use), and the worst row error of the bank against sigsys.fft_caf_host on a 2^18 prefix.
One JSON line per workload."""
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi, sigsys as ss  # noqa: E402

WORKLOADS = {"C9": (np.complex64, 4), "C33": (np.complex64, 16), "C161": (np.complex64, 80), "F33": (np.float32, 16)}
PEAK_TBS = 8.0
N, P, F = 1 << 22, 257, 1024
N_ERR = 1 << 18


def copy_rate_tbs():
    nb = 1 << 30
    a, b = _ffi.DeviceArray(nb // 8, np.complex64), _ffi.DeviceArray(nb // 8, np.complex64)
    L = _ffi.load()
    import ctypes
    for _ in range(3):
        _ffi.check(L.skdsp_memcpy_d2d(ctypes.c_void_p(b.ptr), ctypes.c_void_p(a.ptr), nb))
    _ffi.sync()
    _ffi.timer_start()
    for _ in range(20):
        _ffi.check(L.skdsp_memcpy_d2d(ctypes.c_void_p(b.ptr), ctypes.c_void_p(a.ptr), nb))
    ms = _ffi.timer_stop() / 20
    a.free()
    b.free()
    return 2 * nb / ms / 1e9


def main(argv):
    names = [a for a in argv if a in WORKLOADS] or list(WORKLOADS)
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    per = int(argv[argv.index("--per") + 1]) if "--per" in argv else 4
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    _ffi.init(0)
    copy_tbs = copy_rate_tbs()
    rng = np.random.default_rng(9)
    g = np.conj((rng.standard_normal(P) + 1j * rng.standard_normal(P))[::-1])
    lines = []
    for name in names:
        dt, ns2 = WORKLOADS[name]
        B = 2 * ns2 + 1
        shifts = [j - ns2 for j in range(B)]
        xd = _ffi.DeviceArray(N, dt).fill_noise(7)
        xc = xd if dt == np.complex64 else _ffi.DeviceArray.from_host(xd.to_host().astype(np.complex64))   # the walk's complex copy
        yd = _ffi.DeviceArray(N * B, np.complex64)
        t0 = time.perf_counter()
        bank = _ffi.FirBank(g, shifts, 2 * F, dt)
        bank.filter_dev(xd, yd, N)
        _ffi.sync()
        bank_setup = time.perf_counter() - t0
        t0 = time.perf_counter()
        firs = [_ffi.FirKernel(ss._caf_band_taps(g, s, 2 * F), _ffi.code_of(np.complex64)) for s in shifts]
        create_s = time.perf_counter() - t0
        rows = [yd.window(j * N, N) for j in range(B)]

        def walk():
            for f, r in zip(firs, rows):
                f.filter_dev(xc, r)

        walk()
        _ffi.sync()
        walk_setup = time.perf_counter() - t0
        _ffi.debug_path()
        bank.filter_dev(xd, yd, N)
        path_bank = _ffi.debug_path()
        walk()
        path_walk = _ffi.debug_path()
        _ffi.sync()
        ms_bank, ms_walk, ms_one = [], [], []
        for _ in range(rounds):
            _ffi.timer_start()
            for _ in range(per):
                bank.filter_dev(xd, yd, N)
            ms_bank.append(_ffi.timer_stop() / per)
            with _ffi.option("fir_bank_per", B):      # A/B: ONE band group (every workgroup runs all bands of its tiles)
                _ffi.timer_start()
                for _ in range(per):
                    bank.filter_dev(xd, yd, N)
                ms_one.append(_ffi.timer_stop() / per)
            _ffi.timer_start()
            for _ in range(per):
                walk()
            ms_walk.append(_ffi.timer_stop() / per)
        mb, mw = statistics.median(ms_bank), statistics.median(ms_walk)
        alg = 8 * N * (1 + B)
        # accuracy on a prefix: the bank's rows against the host float64 restatement
        bank.filter_dev(xd, yd, N_ERR, n=N_ERR)
        y = yd.to_host(0, B * N_ERR).reshape(B, N_ERR)
        with contextlib.redirect_stdout(io.StringIO()):
            ref = ss.fft_caf_host(xd.to_host(0, N_ERR), np.conj(g[::-1]), n_fft2=F, n_slice2=ns2, bs=1.0, fs=2.0 * F)[0]
        err = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(y, ref))
        rec = {"workload": name, "dtype": np.dtype(dt).name, "n": N, "taps": P, "n_fft2": F, "slices": B,
               "ms_bank": round(mb, 4), "ms_walk": round(mw, 4), "walk_over_bank": round(mw / mb, 3),
               "ms_bank_one_group": round(statistics.median(ms_one), 4),
               "ms_bank_rounds": [round(v, 4) for v in ms_bank], "ms_walk_rounds": [round(v, 4) for v in ms_walk],
               "alg_bytes": alg, "tbs_bank": round(alg / mb / 1e9, 3), "frac_8tbs": round(alg / mb / 1e9 / PEAK_TBS, 4),
               "copy_tbs": round(copy_tbs, 3), "frac_copy": round(alg / mb / 1e9 / copy_tbs, 4),
               "host_setup_ms_bank": round(bank_setup * 1e3, 1), "host_create_ms_walk": round(create_s * 1e3, 1),
               "host_setup_ms_walk": round(walk_setup * 1e3, 1), "row_err_2p18": err, "path_bank": path_bank, "path_walk": path_walk}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del firs, bank
        if xc is not xd:
            xc.free()
        xd.free()
        yd.free()
    if out_path:
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
