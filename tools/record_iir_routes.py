"""Record which engines every IIR call of a grid runs and what it writes: the table tests/iir_routes/mi355x.txt.

    python tools/record_iir_routes.py [--out FILE] [--commit ID] [--count]

The header carries the device's CU count (the single-pass rule reads it) and the commit recorded; `# design NAME nsec v v v ...` lines
carry the sos rows of every cascade (so that tests/host/iir_route_emul.cpp needs no filter design code).  Then one whitespace-separated
line per call:
    dtype design call arg n options rc engines crc32
dtype is the code of include/skdsp.h; call is filter | state (zi in, zf out) | up | dn | rows (3 rows, stride n + 7); arg is L or M
(else 1); options is name=value,... or -; engines is skdsp_debug_path's list (- if empty); crc32 is zlib.crc32 of the output bytes
(followed by zf for `state`), - where rc != 0 or where two recordings of one commit disagreed.  Only the public device entry points
of _ffi are used, so the script runs unchanged on any commit that has them; tests/test_gpu_iir_routes.py replays the table through run_row.
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
from scipy import signal
from sk_dsp_comm_amd import _ffi

F32, C64, F64, C128 = _ffi.F32, _ffi.C64, _ffi.F64, _ffi.C128
DTYPES = [F32, C64, F64, C128]
DTYPE_NAMES = ["f32", "c64", "f64", "c128"]
N_SHORT = 1000
NROW, ROW_PAD = 3, 7
CUS = 256                      # the CU count the lengths of the single-pass rule are laid out for (the header records the device's own)
TF = {F32: 128, F64: 64, C64: 64, C128: 32}   # the single-pass chunk length per dtype
N_T128 = 96 * 512 * 256 + 1    # D = 16: the first length whose two-pass chunk is 128 samples (the interleaved two-pass kernels apply)


def designs():
    r = 1.0 - 1e-6
    d = {
        "b1": signal.butter(2, 0.3, output="sos"),
        "b2": signal.butter(4, 0.25, output="sos"),
        "e5": signal.ellip(10, 0.4, 70, 0.27, output="sos"),
        "e8": np.load(os.path.join(ROOT, "tests", "golden", "g7_iir_sos.npz"))["sos8"],
        "rep2": np.vstack([signal.butter(2, 0.3, output="sos")] * 2),                   # a double pole pair: the parallel form refuses
        "slow": np.array([[1e-6, 0.0, -1e-6, 1.0, -2.0 * r * np.cos(0.3), r * r]]),     # remembers the whole signal
        "c10": signal.cheby1(20, 0.5, 0.3, output="sos"),                               # 9 .. 12 sections: float32 may not group them
        "b12": signal.butter(24, 0.2, output="sos"),
        "b16": signal.butter(32, 0.3, output="sos"),                                    # grouped 8 + 8
        "c13": signal.cheby1(26, 0.5, 0.3, output="sos"),                               # float32: the float64 twin
        "c20": signal.cheby1(40, 0.5, 0.3, output="sos"),                               # ill-conditioned: the reference's recursion
    }
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in d.items()}


def grid():
    """[(dtype, design, call, arg, n, options)]; options a tuple of (name, value)."""
    rows = []

    def add(dtype, design, call, arg=1, n=N_SHORT, options=()):
        rows.append((dtype, design, call, arg, n, tuple(options)))

    par0, tp1 = ("iir_par", 0), ("iir_two_pass", 1)
    for dt in DTYPES:
        cplx = dt in (C64, C128)
        for name in designs():
            add(dt, name, "filter")
            add(dt, name, "state")
            add(dt, name, "up", 2)
            add(dt, name, "dn", 3)
            add(dt, name, "rows")
        for name in ("e8", "b16"):
            for L in (3, 4, 5, 12):
                add(dt, name, "up", L)
            for M in (2, 4, 5, 96, 4097):
                add(dt, name, "dn", M, n=3 * 4097 if M == 4097 else N_SHORT)
        if dt in (F32, C64):
            for name in ("b2", "slow", "c13", "c20"):
                add(dt, name, "up", 3)
                add(dt, name, "dn", 2)
                add(dt, name, "dn", 4097, n=3 * 4097)
        for name in ("b2", "e8", "rep2", "slow", "b16"):
            add(dt, name, "filter", options=(par0,))
            add(dt, name, "up", 2, options=(par0,))
            add(dt, name, "dn", 3, options=(par0,))
            add(dt, name, "rows", options=(par0,))
        for name in ("e8", "slow"):
            add(dt, name, "filter", options=(par0, tp1))
            add(dt, name, "dn", 3, options=(par0, tp1))
        for name in ("e8", "b2"):
            add(dt, name, "filter", options=(("iir_two_pass", -1),))
        if cplx:
            for name in ("e8", "rep2", "b16"):
                add(dt, name, "filter", options=(("iir_planar", 1),))
                add(dt, name, "up", 2, options=(("iir_planar", 1),))
                add(dt, name, "dn", 3, options=(("iir_planar", 1),))
        for name in ("e8", "b16"):
            add(dt, name, "dn", 3, options=(("iir_dn_full", 1),))
            add(dt, name, "up", 2, options=(("iir_up_fused", 0),))
        for name in ("e8", "rep2"):
            add(dt, name, "filter", options=(("iir_no_mfma", 1),))
            add(dt, name, "state", options=(("iir_no_mfma", 1),))
        # the single-pass rule n >= Tf * 256 * CUs: where the parallel form is switched off, where it refuses, and the complex64 policy
        edge = TF[dt] * 256 * CUS
        for n in (edge - 1, edge):
            add(dt, "e8", "filter", n=n, options=(par0,))
            add(dt, "rep2", "filter", n=n)
            add(dt, "e8", "filter", n=n, options=(par0, ("iir_two_pass", -1)))
        add(dt, "e8", "dn", 3, n=edge, options=(par0,))
        add(dt, "slow", "filter", n=edge, options=(par0,))
        # the chunk length of the two-pass scan reaches 128
        if dt != F64:
            for n in (N_T128 - 1, N_T128):
                add(dt, "e8", "filter", n=n, options=(par0, tp1))   # (six scan levels: the per-thread K1 either way)
                add(dt, "b2", "filter", n=n, options=(par0, tp1))
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def n_out_of(call, arg, n):
    return n * arg if call == "up" else n // arg if call == "dn" else NROW * (n + ROW_PAD) if call == "rows" else n


def format_options(options):
    return ",".join("%s=%d" % o for o in options) if options else "-"


def parse_row(line):
    """A line of the table -> (row as grid() gives it, rc, engines, crc or None)."""
    f = line.split()
    options = () if f[5] == "-" else tuple((kv.split("=")[0], int(kv.split("=")[1])) for kv in f[5].split(","))
    row = (int(f[0]), f[1], f[2], int(f[3]), int(f[4]), options)
    return row, int(f[6]), ([] if f[7] == "-" else f[7].split(",")), (None if f[8] == "-" else int(f[8]))


def format_row(row, rc, engines, crc):
    return "%d %s %s %d %d %s %d %s %s" % (row[:5] + (format_options(row[5]), rc, ",".join(engines) if engines else "-",
                                                      "-" if crc is None else str(crc)))


class Runner:
    """Device buffers and handles shared by the rows: one random input per signal dtype, one output buffer, one handle per (dtype, design)."""

    def __init__(self, rows):
        self.lib = _ffi.load()
        self.max_in = max(NROW * (r[4] + ROW_PAD) if r[2] == "rows" else r[4] for r in rows)
        self.y_bytes = max(n_out_of(r[2], r[3], r[4]) * np.dtype(_ffi.np_of(r[0])).itemsize for r in rows)
        self.y = _ffi.DeviceArray(self.y_bytes // 4 + 16, np.float32)
        self.x, self.handles, self.sos = {}, {}, designs()

    def input_of(self, dtype):
        if dtype not in self.x:
            npdt = _ffi.np_of(dtype)
            block = np.random.default_rng(2000 + dtype).standard_normal(self.max_in)
            if np.dtype(npdt).kind == "c":   # (a generator per component: the first n samples do not depend on the longest row of the run)
                block = (block + 1j * np.random.default_rng(3000 + dtype).standard_normal(self.max_in)) / np.sqrt(2.0)
            self.x[dtype] = _ffi.DeviceArray.from_host(block.astype(npdt))
        return self.x[dtype]

    def handle_of(self, dtype, design):
        if (dtype, design) not in self.handles:
            self.handles[(dtype, design)] = _ffi.IirKernel(dtype, sos=self.sos[design])
        return self.handles[(dtype, design)]

    def run_row(self, row):
        """-> (rc, engines, crc or None)"""
        dtype, design, call, arg, n, options = row
        lib = self.lib
        esz = np.dtype(_ffi.np_of(dtype)).itemsize
        n_out = n_out_of(call, arg, n)
        xd = self.input_of(dtype)
        k = self.handle_of(dtype, design)
        old = [(name, _ffi.set_option(name, value)) for name, value in options]
        zf = None
        try:
            _ffi.check(lib.skdsp_memset(ctypes.c_void_p(self.y.ptr), 0, n_out * esz))
            x, y, h = ctypes.c_void_p(xd.ptr), ctypes.c_void_p(self.y.ptr), ctypes.c_void_p(k.h)
            _ffi.debug_path()
            if call == "filter":
                rc = lib.skdsp_iir_filter_dev(h, x, n, y)
            elif call == "state":
                zi = 0.01 * np.cos(np.arange(k.state_len(), dtype=np.float64))
                zf = np.zeros(k.state_len())
                rc = lib.skdsp_iir_filter_state_dev(h, x, n, _ffi._ptr(zi), _ffi._ptr(zf), y)
            elif call == "up":
                rc = lib.skdsp_iir_up_dev(h, x, n, arg, y)
            elif call == "dn":
                rc = lib.skdsp_iir_dn_dev(h, x, n, arg, y)
            else:
                rc = lib.skdsp_iir_filter_rows_dev(h, x, n, NROW, n + ROW_PAD, n + ROW_PAD, y)
            engines = _ffi.debug_path()
            if rc in (-2, -3, -4):   # no device, no memory, SKDSP_ERR_HIP: nothing more runs on this device
                raise _ffi.SkdspError("HIP error in row %r: %s" % (row, lib.skdsp_last_error().decode("utf-8", "replace")))
            _ffi.sync()
            crc = None
            if rc == 0:
                out = np.empty(n_out * esz, dtype=np.uint8)
                _ffi.check(lib.skdsp_memcpy_d2h(_ffi._ptr(out), y, out.nbytes))
                crc = zlib.crc32(out)
                if zf is not None:
                    crc = zlib.crc32(zf.tobytes(), crc)
        finally:
            for name, value in reversed(old):
                _ffi.set_option(name, value)
        return rc, engines, crc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="iir_routes.txt")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--count", action="store_true", help="print the size of the grid and leave")
    a = ap.parse_args()
    rows = grid()
    if a.count:
        print("%d rows, %d beyond %d samples" % (len(rows), sum(1 for r in rows if r[4] > 3 * 4097), 3 * 4097))
        return
    _ffi.init(0)
    info = _ffi.device_info()
    run = Runner(rows)
    with open(a.out, "w") as f:
        f.write("# cus=%d commit=%s device=%s\n" % (info["compute_units"], a.commit, info["name"].replace(" ", "_")))
        for name, sos in designs().items():
            f.write("# design %s %d %s\n" % (name, sos.shape[0], " ".join("%.17g" % v for v in sos.ravel())))
        for j, row in enumerate(rows):
            f.write(format_row(row, *run.run_row(row)) + "\n")
            if j % 50 == 0:
                f.flush()
                print("%d / %d" % (j, len(rows)), flush=True)
    print("recorded %d rows" % len(rows))


if __name__ == "__main__":
    main()
