"""Record which engine every FIR call of a grid runs and what it writes: the table tests/fir_routes/mi355x.txt.

    python tools/record_fir_routes.py --out FILE [--commit ID] [--slice I/K]

One whitespace-separated line per call:
    dtype taps_complex set_algo ntaps L M n n_hist y_offset options rc engines crc32
dtype / set_algo are the codes of include/skdsp.h; L = M = 1 is .filter, M = 1 .up, L = 1 .dn, else the fused L / M; y_offset counts elements;
options is name=value,... or -; engines is skdsp_debug_path's list (- if empty); crc32 is zlib.crc32 of the output bytes (- where rc != 0).
The header line carries the device's CU count (the cost model reads it) and the commit recorded.  Only the public device entry points of
_ffi are used, so the script runs unchanged on any commit that has them; tests/test_gpu_fir_routes.py replays the table through run_row.
"""
import argparse
import ctypes
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
import numpy as np
from sk_dsp_comm_amd import _ffi

F32, C64, F64, C128 = _ffi.F32, _ffi.C64, _ffi.F64, _ffi.C128
CLASSES = [(F32, 0), (C64, 0), (F64, 0), (C128, 0), (C64, 1), (C128, 1)]   # (signal dtype, complex taps)
CLASS_NAMES = ["f32", "c64", "f64", "c128", "c64_ctaps", "c128_ctaps"]

# tap counts on both sides of every rule of the dispatch; a group shares its thinning so that both sides meet the same rates
TAP_GROUPS = [[9], [23, 24], [47, 48], [96], [127, 128], [176, 177], [192, 193], [512], [1024], [1536, 1537], [2049, 2050], [3072],
              [4097, 4098], [6144], [12288]]
UPS = [2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 24]
DNS = [2, 3, 4, 5, 6, 8, 12, 16, 24, 100]
RATIOS = [(4, 3), (3, 2), (12, 5), (5, 12), (7, 4), (16, 3)]
RATES = [(1, 1)] + [(L, 1) for L in UPS] + [(1, M) for M in DNS] + RATIOS
N_RAGGED, N_MID = 12289, (1 << 17) + 3
LARGE_OUT, MAX_IN = 1 << 25, 1 << 28
LARGE_TAPS = {48, 128, 193, 512, 1024, 1537, 3072, 6144}
NOISE_PERIOD = (1 << 20) + 7   # the input is this many random samples, repeated


def n_large(L, M):
    return min(LARGE_OUT * M // L, MAX_IN)


def n_out_of(L, M, n):
    return n if L == 1 and M == 1 else (n * L) // M


def grid():
    """[(dtype, taps_complex, algo, ntaps, L, M, n, n_hist, y_off, options)]; options a tuple of (name, value)."""
    rows = []

    def add(cls, ntaps, L, M, n, n_hist=0, y_off=0, algo=0, options=()):
        rows.append((cls[0], cls[1], algo, ntaps, L, M, n, n_hist, y_off, tuple(options)))

    for cls in CLASSES:
        for gi, group in enumerate(TAP_GROUPS):
            for ntaps in group:
                for ri, (L, M) in enumerate(RATES):
                    plain = L == 1 and M == 1
                    if plain:
                        add(cls, ntaps, 1, 1, 100)          # from rest, fewer samples than taps: a head
                    if plain or (gi + ri) % 4 == 0:
                        add(cls, ntaps, L, M, N_RAGGED)     # three ragged tiles of every tile engine
                    if plain or (gi + ri) % 4 == 2:
                        add(cls, ntaps, L, M, N_MID)
                    if ntaps in LARGE_TAPS and (plain or (gi + ri) % 4 == 1):
                        add(cls, ntaps, L, M, n_large(L, M))
        for ntaps in (9, 512, 4098):   # short calls from rest of the rate changers
            for L, M in ((4, 1), (1, 3), (3, 2), (1, 100)):
                add(cls, ntaps, L, M, 100)
        # strides the polyphase launcher's window does not hold: the decimating store, the full-rate filter and a strided copy, the walk with dec = M
        for M in (5000, 20000, 40000):
            add(cls, 400, 1, M, N_MID)
            add(cls, 400, 1, M, N_MID, options=(("dn_no_ols", 1),))
        add(cls, 1000, 3, 4000, 6000)
        add(cls, 1000, 3, 4000, N_MID)
        # history in front of x
        for ntaps, L, M in ((193, 1, 1), (1024, 1, 1), (1024, 4, 1), (1024, 1, 3), (512, 3, 2), (6144, 1, 1)):
            add(cls, ntaps, L, M, N_RAGGED, n_hist=2000)
        # tap segments (.dn by 3: whole output periods are 3 inputs) with a partial history that is / is not a multiple of M / gcd, and a complete one
        for n_hist in (300, 301, 12287):
            add(cls, 12288, 1, 3, N_MID, n_hist=n_hist)
        add(cls, 12288, 3, 2, N_MID, n_hist=300)
        add(cls, 12288 * 3, 3, 2, N_MID, n_hist=300)
        add(cls, 12288 * 3, 3, 2, N_MID, n_hist=301)
        # a tap segment whose stride the polyphase launcher does not hold: the full-rate filter cannot use workspace slot 2 there.  (float64 signals: one
        # output period, 4000 taps, is longer than a launch takes -- no segment length serves such a call)
        if cls[0] in (F32, C64):
            add(cls, 12288, 1, 4000, N_MID)
            add(cls, 12288, 1, 4000, N_MID, options=(("dn_no_ols", 1),))
    # float32: y one element off an 8-byte boundary (the pairs forms)
    for ntaps in (512, 3072):
        for L in (2, 4, 7, 8, 9, 13):
            for n in (N_MID, n_large(L, 1)):
                add(CLASSES[0], ntaps, L, 1, n, y_off=1)
                add(CLASSES[2], ntaps, L, 1, n, y_off=1)
    # options forced, on a reduced shape set
    up_shapes = [(96, 2), (512, 2), (512, 3), (1024, 4), (512, 7), (1024, 8), (3072, 12), (1024, 13), (6144, 16), (12288, 24)]
    dn_shapes = [(512, 2), (512, 3), (1024, 4), (3072, 3), (1024, 6), (2050, 8), (1024, 16)]
    up_opts = [("fir_up4k", 0), ("fir_up4k", 2), ("fir_up2k", 0), ("fir_up2k", 2), ("fir_up_rep", 0), ("fir_up_rep", 2), ("fir_algo", 1), ("fir_algo", 2),
               ("fir_up_ols_min", 0), ("fir_up_ols_min", -2), ("fir_up_rows_min", 0), ("fir_up_rows_min", 4), ("fir_up_pair", 0), ("fir_bx", 0), ("fir_mm", 0)]
    dn_opts = [("fir_dn4k", 0), ("fir_dn4k", 2), ("fir_algo", 1), ("fir_algo", 2), ("fir_dn_fold", 0), ("fir_bx", 0), ("fir_mm", 0), ("dn_no_ols", 1)]
    f64_opts = {"fir_algo", "dn_no_ols", "fir_up_ols_min", "fir_up_rows_min", "fir_up_pair", "fir_mm", "fir_updn_fused"}   # what the float64 side reads
    for cls in CLASSES[:3]:
        if cls[0] == F64:
            up_opts = [o for o in up_opts if o[0] in f64_opts]
            dn_opts = [o for o in dn_opts if o[0] in f64_opts]
        for o in up_opts:
            for ntaps, L in up_shapes:
                for n in (N_MID, n_large(L, 1)):
                    if n == N_MID or L in (4, 12):
                        add(cls, ntaps, L, 1, n, options=(o,))
        for o in dn_opts:
            for ntaps, M in dn_shapes:
                for n in (N_MID, n_large(1, M)):
                    if n == N_MID or M in (3, 8):
                        add(cls, ntaps, 1, M, n, options=(o,))
        for o in (("fir_algo", 1), ("fir_algo", 2), ("fir_bx", 0), ("fir_mm", 0)):
            for ntaps in (48, 193, 1024):
                add(cls, ntaps, 1, 1, N_MID, options=(o,))
        for o in (("fir_updn_fused", 0), ("fir_up_ols_min", 0), ("fir_up_ols_min", -2), ("fir_algo", 1), ("fir_bx", 0)):
            for ntaps, L, M in ((1024, 4, 3), (3072, 3, 2), (6144, 12, 5), (3072, 16, 3)):
                for n in (N_MID, n_large(L, M)):
                    add(cls, ntaps, L, M, n, options=(o,))
    # skdsp_fir_set_algo on the handle
    for cls in CLASSES:
        for algo in (1, 2):
            for ntaps, L, M in ((48, 1, 1), (1024, 1, 1), (12288, 1, 1), (1024, 1, 2), (1024, 1, 3), (1024, 1, 8), (1024, 4, 1), (1024, 4, 3)):
                add(cls, ntaps, L, M, N_MID, algo=algo)
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def format_options(options):
    return ",".join("%s=%d" % o for o in options) if options else "-"


def parse_row(line):
    """A line of the table -> (row as grid() gives it, rc, engines, crc or None)."""
    f = line.split()
    options = () if f[9] == "-" else tuple((kv.split("=")[0], int(kv.split("=")[1])) for kv in f[9].split(","))
    row = tuple(int(v) for v in f[:9]) + (options,)
    return row, int(f[10]), ([] if f[11] == "-" else f[11].split(",")), (None if f[12] == "-" else int(f[12]))


def firwin_lowpass(ntaps, cutoff):
    """A Hamming-windowed low-pass of unit DC gain (bench.firwin_lowpass)."""
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = cutoff * np.sinc(cutoff * m) * np.hamming(ntaps)
    return h / np.sum(h)


class Runner:
    """Device buffers and handles shared by the rows: one periodic random input per signal dtype (as long as the longest call
    asked for), one output buffer, one handle per (dtype, taps)."""

    HEAD = 65536   # samples kept in front of x[0] for n_hist

    def __init__(self, max_in, max_out_bytes):
        self.lib = _ffi.load()
        self.max_in = int(max_in)
        self.x = {}
        self.y_bytes = int(max_out_bytes)
        self.y = _ffi.DeviceArray(self.y_bytes // 4 + 16, np.float32)
        self.handles = {}

    def input_of(self, dtype):
        if dtype not in self.x:
            npdt = _ffi.np_of(dtype)
            rng = np.random.default_rng(1000 + dtype)
            block = rng.standard_normal(NOISE_PERIOD)
            if np.dtype(npdt).kind == "c":
                block = (block + 1j * rng.standard_normal(NOISE_PERIOD)) / np.sqrt(2.0)
            block = block.astype(npdt)
            total = self.HEAD + self.max_in
            xd = _ffi.DeviceArray(total, npdt)
            for at in range(0, total, NOISE_PERIOD):
                xd.write(block[:min(NOISE_PERIOD, total - at)], at)
            self.x[dtype] = xd
        return self.x[dtype]

    def handle_of(self, dtype, taps_complex, ntaps):
        key = (dtype, taps_complex, ntaps)
        if key not in self.handles:
            if len(self.handles) > 64:
                self.handles.clear()
            rng = np.random.default_rng(7 * ntaps + taps_complex)
            b = firwin_lowpass(ntaps, 0.2)
            if taps_complex:
                b = b * np.exp(2j * np.pi * rng.uniform() + 0.3j * np.arange(ntaps))
            self.handles[key] = _ffi.FirKernel(b, dtype)
        return self.handles[key]

    def run_row(self, row):
        """-> (rc, engines, crc or None)"""
        dtype, taps_complex, algo, ntaps, L, M, n, n_hist, y_off, options = row
        lib = self.lib
        esz = np.dtype(_ffi.np_of(dtype)).itemsize
        n_out = n_out_of(L, M, n)
        if n > self.max_in or n_hist > self.HEAD or (n_out + y_off) * esz > self.y_bytes:
            raise ValueError("row %r does not fit the runner's buffers" % (row,))
        xd = self.input_of(dtype)
        k = self.handle_of(dtype, taps_complex, ntaps)
        k.set_algo(algo)
        old = [(name, _ffi.set_option(name, value)) for name, value in options]
        try:
            _ffi.check(lib.skdsp_memset(ctypes.c_void_p(self.y.ptr), 0, (n_out + y_off) * esz))
            x = ctypes.c_void_p(xd.ptr + self.HEAD * esz)
            y = ctypes.c_void_p(self.y.ptr + y_off * esz)
            h = ctypes.c_void_p(k.h)
            _ffi.debug_path()
            if L == 1 and M == 1:
                rc = lib.skdsp_fir_filter_dev(h, x, n, n_hist, y)
            elif M == 1:
                rc = lib.skdsp_fir_up_dev(h, x, n, n_hist, L, y)
            elif L == 1:
                rc = lib.skdsp_fir_dn_dev(h, x, n, n_hist, M, y)
            else:
                rc = lib.skdsp_fir_updn_dev(h, x, n, n_hist, L, M, y)
            engines = _ffi.debug_path()
            if rc in (-2, -3, -4):   # no device, no memory, SKDSP_ERR_HIP: nothing more runs on this device
                raise _ffi.SkdspError("HIP error in row %r: %s" % (row, lib.skdsp_last_error().decode("utf-8", "replace")))
            _ffi.sync()
            crc = None
            if rc == 0:
                out = np.empty(n_out * esz, dtype=np.uint8)
                _ffi.check(lib.skdsp_memcpy_d2h(_ffi._ptr(out), y, out.nbytes))
                crc = zlib.crc32(out)
        finally:
            for name, value in reversed(old):
                _ffi.set_option(name, value)
        return rc, engines, crc


def runner_for(rows):
    max_in = max(r[6] for r in rows)
    max_out = max((n_out_of(r[4], r[5], r[6]) + r[8]) * np.dtype(_ffi.np_of(r[0])).itemsize for r in rows)
    return Runner(max_in, max_out)


def format_row(row, rc, engines, crc):
    return "%d %d %d %d %d %d %d %d %d %s %d %s %s" % (row[:9] + (format_options(row[9]), rc, ",".join(engines) if engines else "-",
                                                                   "-" if crc is None else str(crc)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--slice", default="0/1", help="I/K: every K-th row from the I-th on")
    ap.add_argument("--count", action="store_true", help="print the size of the grid and leave")
    a = ap.parse_args()
    rows = grid()
    if a.count:
        large = sum(1 for r in rows if r[6] > N_MID)
        print("%d rows, %d beyond %d samples" % (len(rows), large, N_MID))
        return
    i, k = (int(v) for v in a.slice.split("/"))
    rows = rows[i::k]
    _ffi.init(0)
    info = _ffi.device_info()
    run = runner_for(rows)
    with open(a.out, "w") as f:
        f.write("# cus=%d commit=%s device=%s\n" % (info["compute_units"], a.commit, info["name"].replace(" ", "_")))
        for j, row in enumerate(rows):
            f.write(format_row(row, *run.run_row(row)) + "\n")
            if j % 100 == 0:
                f.flush()
                print("%d / %d" % (j, len(rows)), flush=True)
    print("recorded %d rows" % len(rows))


if __name__ == "__main__":
    main()
