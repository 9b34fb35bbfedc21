"""A device call reads its own input window and nothing else.

Every *_dev entry point takes a pointer into a larger device buffer, a sample count n and (FIR) a history length n_hist, and the
host chunk pipeline, the sharded drivers, filter_stream and every DeviceArray.window caller rely on it reading exactly
x[-n_hist .. n-1]: what lies in front of or behind that window must not change one output bit.  The loaders' guard
(g >= -n_hist && g < n) is written out in every engine; the rest of the suite surrounds its windows with zeros, which is what a
from-rest call assumes in front of x[0] and what a causal filter cannot see behind x[n-1], so a guard that is off by a tile, a block
or a vector passes there.  Here every engine runs on a window inside [16384 | x | 16384] (more than the largest tile, 8192, plus the
largest overlap, 4096: an over-read of a whole tile still lands in the pad, inside the allocation) with the pads filled three ways --
zeros, loud finite values (~2^20: a leak into a transform costs the tile its 1e-6, a leak into the fp16-piece kernel's window maximum
changes its scale) and NaN (a leak trips the non-finite recompute path or poisons an output) -- and must write the same BYTES each
time, run the same engines, leave the guard words around its output alone, and with zero pads hold the library's contract against a
float64 reference computed here (1e-6 of the output's peak for float32 / complex64, 1e-10 for float64 / complex128, as
test_gpu_fuzz._check).  Two window offsets: 16-byte aligned (the vector fast paths) and one element further (the edge paths).  FIR
calls run from rest, behind a partial history (the first chunks of the host pipeline and of a sharded step) and behind a full one.

One line per case, offset and history is printed: the engines that ran and the error against the reference."""
import contextlib
import ctypes
import math
import os

import numpy as np
import pytest
from scipy import signal

from conftest import GOLDEN
from _pads import loud
from sk_dsp_comm_amd import _ffi, multirate_helper as mrh, sigsys as ss
from test_farrow_cpu import farrow_restated

pytestmark = pytest.mark.gpu

PAD = 16384        # elements in front of and behind every input window
GUARD = 64         # guard words on each side of every output
SENTINEL = 7.25
OFFSETS = (0, 1)   # window start: PAD (16-byte aligned) and PAD + 1 (element-aligned only); y moves along
FILLS = ("zeros", "loud", "nan")


def _single(dt):
    dt = np.dtype(dt)
    return dt.itemsize // (2 if dt.kind == "c" else 1) == 4


def _wide(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def _tol(dt):
    return 1e-6 if _single(dt) else 1e-10


def _noise(seed, n, dt):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dt)


def _fill(kind, count, dt, first=0):
    """`count` pad elements of `dt` for positions first .. first + count - 1 of a buffer."""
    dt = np.dtype(dt)
    if kind == "zeros":
        return np.zeros(count, dt)
    if kind == "nan":
        return np.full(count, np.nan + 1j * np.nan if dt.kind == "c" else np.nan, dtype=dt)
    return loud(count, dt, first)


def _rel(y, ref, bound=0.0):
    """max |y - ref| over the output's peak (or 1 % of the forward bound, whichever is larger: test_gpu_fuzz._check)."""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    scale = max(float(np.max(np.abs(ref))), 1e-2 * bound)
    return float(np.max(np.abs(y - ref))) / scale


def footprint(what, engine, body, n_hist, n_y, call, ref, tol, *, y_dtype=None, outside=None, y_written=None, fills=FILLS, offsets=OFFSETS,
              bound=0.0, exact=False, check=None):
    """Runs `call(x_window, y_window)` -- one *_dev call; whatever it returns (end states, ...) is compared along with the output --
    on `body` (n_hist history samples first) inside [PAD | body | PAD] and [GUARD | y | GUARD], at every offset and with every pad fill,
    the first fill twice.  outside: the elements of `body` that belong to no window (the gaps between strided rows), filled like the pads;
    y_written: the elements of y the call writes (all by default), the others must keep the sentinel.
    ref / tol / bound: the float64 reference of the first fill (zeros) and the contract; exact: bit for bit instead;
    check(y, path): a contract of the caller's own instead, which it asserts itself (the error it returns is printed).  Returns the worst error against the reference."""
    body = np.ascontiguousarray(body)
    dt = body.dtype
    y_dtype = np.dtype(dt if y_dtype is None else y_dtype)
    nb = body.size
    inside = np.ones(nb, bool) if outside is None else ~outside
    problems, worst = [], 0.0
    xbuf = _ffi.DeviceArray(2 * PAD + nb + len(offsets), dt)
    ybuf = _ffi.DeviceArray(2 * GUARD + n_y + len(offsets), y_dtype)
    sent = np.full(ybuf.n, SENTINEL, dtype=y_dtype)
    try:
        for off in offsets:
            x0, y0 = PAD + off, GUARD + off
            runs = []
            for kind in (fills[0],) + tuple(fills):
                image = _fill(kind, xbuf.n, dt)
                image[x0:x0 + nb][inside] = body[inside]
                xbuf.write(image)
                ybuf.write(sent)
                _ffi.debug_path()
                with np.errstate(all="ignore"):
                    extra = call(xbuf.window(x0 + n_hist, nb - n_hist), ybuf.window(y0, n_y))
                path = _ffi.debug_path()
                got = ybuf.to_host()
                y = got[y0:y0 + n_y]
                held = np.ones(ybuf.n, bool)
                held[y0:y0 + n_y] = False if y_written is None else ~y_written
                if not np.array_equal(got[held], sent[held]):
                    problems.append("offset %d, pads %s: guard words around the output overwritten" % (off, kind))
                runs.append((kind, y.copy(), path, None if extra is None else np.asarray(extra).tobytes()))
            (_, y_a, path_a, extra_a), second = runs[0], runs[1]
            tag = "%s: offset %d, n_hist %d, %s" % (what, off, n_hist, ",".join(path_a) or "-")
            if second[1].tobytes() != y_a.tobytes() or second[3] != extra_a:
                problems.append("%s: two runs on the same buffer differ (%d elements, by up to %.3g)" % (
                    tag, int(np.sum(second[1] != y_a)), float(np.nanmax(np.abs(second[1] - y_a)))))
            for kind, y, path, extra in runs[1:]:
                if path != path_a:
                    problems.append("%s: pads %s ran %s" % (tag, kind, path))
                if kind != fills[0] and (y.tobytes() != y_a.tobytes() or extra != extra_a):
                    d = np.flatnonzero((y != y_a) & ~(np.isnan(y) & np.isnan(y_a)))
                    problems.append("%s: pads %s change the result: %d of %d outputs differ, first at %s, last at %s%s" % (
                        tag, kind, d.size, y.size, d[:1], d[-1:], "" if extra == extra_a else "; the returned state differs"))
            if engine is not None and not all(e in path_a for e in ([engine] if isinstance(engine, str) else engine)):
                problems.append("%s: meant for %s" % (tag, engine))
            yw = y_a[y_written] if y_written is not None else y_a
            if check is not None:
                try:
                    err = check(yw, path_a)
                except AssertionError as e:
                    problems.append("%s: %s" % (tag, e))
                    err = float("nan")
            elif exact:
                err = 0.0 if np.array_equal(yw, ref) else float("inf")
            else:
                err = _rel(yw, ref, bound)
            print("%s: error %.3g" % (tag, err))
            worst = max(worst, err) if err == err else worst
            if check is None and not err <= (0.0 if exact else tol):
                problems.append("%s: error %.3g against the float64 reference, contract %.1g" % (tag, err, tol))
    finally:
        xbuf.free()
        ybuf.free()
    assert not problems, "\n".join(problems)
    return worst


def _options(opts):
    st = contextlib.ExitStack()
    for name, value in opts.items():
        st.enter_context(_ffi.option(name, value))
    return st


# ================================================================================================================== FIR
def _tile_n(v):
    """Two full tiles of v outputs and a ragged one."""
    return 2 * v + v // 3


def _fir(name, engine, dt, ntaps, mode, n, L=1, M=1, opts=None, ctaps=False, hists=("rest", "partial", "full")):
    return dict(name=name, engine=engine, dt=dt, ntaps=ntaps, mode=mode, n=n, L=L, M=M, opts=opts or {}, ctaps=ctaps, hists=hists)


WALK = {"fir_up_ols_min": -2, "fir_up4k": 0, "fir_up_rep": 0}
C64, F32, F64, C128 = np.complex64, np.float32, np.float64, np.complex128

# the tile sizes: fir_ols / the walk 8192 points with the overlap in steps of 512; fir_ols64 and fir_up4k / fir_dn4k 4096 in steps of 256;
# fir_up2k 2048 in steps of 64.  The window kernels (fir_bx, fir_mm, fir_direct): 12289 or 20001 samples.
FIR_CASES = [
    # ---- .filter
    _fir("ols_c64", "fir_ols", C64, 1024, "filter", _tile_n(7168)),
    _fir("ols_f32", "fir_ols", F32, 1024, "filter", _tile_n(7168)),                       # (the real-pair tile)
    _fir("ols_4097_c64", "fir_ols", C64, 4097, "filter", _tile_n(4096)),
    _fir("bx_f32", "fir_bx", F32, 127, "filter", 12289),
    _fir("bx_c64", "fir_bx", C64, 127, "filter", 20001),
    _fir("mm_f32", "fir_mm", F32, 127, "filter", 12289, opts={"fir_bx": 0}),
    _fir("mm_c64", "fir_mm", C64, 127, "filter", 20001, opts={"fir_bx": 0}),
    _fir("direct_f32", "fir_direct", F32, 127, "filter", 12289, opts={"fir_mm": 0}),
    _fir("direct_c64", "fir_direct", C64, 127, "filter", 20001, opts={"fir_mm": 0}),
    _fir("direct_ctaps_c64", "fir_direct", C64, 33, "filter", 20001, ctaps=True),
    _fir("direct_f64", "fir_direct", F64, 48, "filter", 12289, opts={"fir_mm": 0}),
    _fir("mm_f64", "fir_mm", F64, 48, "filter", 12289),
    _fir("ols64_f64", "fir_ols64", F64, 1024, "filter", _tile_n(3072), opts={"fir_algo": 2}),
    _fir("ols64_c128", "fir_ols64", C128, 1024, "filter", _tile_n(3072), opts={"fir_algo": 2}),
    _fir("parts_c64", "fir_ols", C64, 5000, "filter", _tile_n(4096)),                     # (tap segments: 4096 + 904 taps)
    _fir("head_700", "fir_direct", C64, 1024, "filter", 700, hists=("rest",)),                    # (from rest, fewer samples than taps)
    _fir("head_500", "fir_direct", C64, 1024, "filter", 500, hists=("rest",)),                    # (... on the filter's first 512 taps)
    # ---- .up
    _fir("up12_bx", "fir_bx", C64, 512, "up", 12289, L=12),
    _fir("up4_rep_c64", "fir_ols_rep", C64, 1024, "up", -(-_tile_n(7168) // 4), L=4, opts={"fir_up_rep": 2}),
    _fir("up4_rep_f32", "fir_ols_rep", F32, 1024, "up", -(-_tile_n(7168) // 4), L=4, opts={"fir_up_rep": 2}),
    _fir("up3_4k_c64_g4", "fir_up4k", C64, 768, "up", _tile_n(3840), L=3, opts={"fir_up4k": 2, "fir_up4k_group": 4}),
    _fir("up3_4k_c64_g2", "fir_up4k", C64, 768, "up", _tile_n(3840), L=3, opts={"fir_up4k": 2, "fir_up4k_group": 2}),
    _fir("up3_4k_f32_g4", "fir_up4k", F32, 768, "up", _tile_n(3840), L=3, opts={"fir_up4k": 2, "fir_up4k_group": 4}),
    _fir("up3_4k_f32_g2", "fir_up4k", F32, 768, "up", _tile_n(3840), L=3, opts={"fir_up4k": 2, "fir_up4k_group": 2}),
    _fir("up9_2k_c64", "fir_up2k", C64, 2304, "up", _tile_n(1792), L=9, opts={"fir_up4k": 2, "fir_up2k": 2}),
    _fir("up3_walk_strided", "fir_ols_up", C64, 768, "up", _tile_n(7680), L=3, opts=WALK),
    _fir("up3_walk_rows", "fir_ols_up", C64, 768, "up", _tile_n(7680), L=3, opts=dict(WALK, fir_up_rows_min=2)),
    _fir("up4_walk_pairs_f32", "fir_ols_up", F32, 1024, "up", _tile_n(7680), L=4, opts=WALK),
    _fir("up7_walk_pairs_f32", "fir_ols_up", F32, 1792, "up", _tile_n(7680), L=7, opts=WALK),
    _fir("up4_ols64_f64", "fir_ols64_up", F64, 1024, "up", _tile_n(3840), L=4, opts={"fir_up_ols_min": -2}),
    # ---- .dn (n % M != 0 everywhere: the trailing samples are dropped)
    _fir("dn12_bx", "fir_bx", C64, 512, "dn", 20001, M=12),
    _fir("dn3_store_c64", "fir_ols", C64, 1024, "dn", _tile_n(7168) + 1, M=3, opts={"fir_dn4k": 0}),
    _fir("dn4_fold_c64", "fir_ols", C64, 1024, "dn", _tile_n(7168), M=4),
    _fir("dn4_fold_f32", "fir_ols", F32, 1024, "dn", _tile_n(7168), M=4),
    _fir("dn3_4k_c64", "fir_dn4k", C64, 1024, "dn", _tile_n(3584) * 3 + 1, M=3, opts={"fir_dn4k": 2}),
    _fir("dn3_4k_f32", "fir_dn4k", F32, 1024, "dn", _tile_n(3584) * 3 + 1, M=3, opts={"fir_dn4k": 2}),
    _fir("dn4_4k_c64", "fir_dn4k", C64, 1024, "dn", _tile_n(3840) * 4 + 1, M=4, opts={"fir_dn4k": 2}),
    _fir("dn3_ols64_f64", "fir_ols64", F64, 512, "dn", _tile_n(3584), M=3),
    # ---- L / M
    _fir("updn43_bx", "fir_bx", C64, 512, "updn", 20001, L=4, M=3),
    _fir("updn43_walk", "fir_ols_up", C64, 2048, "updn", _tile_n(7680), L=4, M=3, opts={"fir_up_ols_min": -2}),
    _fir("updn43_walk_unfused", "fir_ols_up", C64, 2048, "updn", _tile_n(7680), L=4, M=3, opts={"fir_up_ols_min": -2, "fir_updn_fused": 0}),
]


def _taps(c):
    f = max(c["L"], c["M"])
    b = signal.firwin(c["ntaps"], 0.4 if f == 1 else 0.9 / f)
    return b * np.exp(0.3j * np.arange(c["ntaps"])) if c["ctaps"] else b


def _hist_len(c, kind):
    L, M, ntaps = c["L"], c["M"], c["ntaps"]
    if kind == "rest":
        return 0
    if kind == "full":
        return -(-(ntaps - 1) // L)
    q = M // math.gcd(L, M)   # (a partial history of a decimating call: whole output periods, fir_parts_history_ok)
    return 37 if q == 1 else (36 // q) * q


def _fir_n_out(c, n=None):
    n = c["n"] if n is None else n
    return {"filter": n, "up": n * c["L"], "dn": n // c["M"], "updn": (n * c["L"]) // c["M"]}[c["mode"]]


def _fir_ref(b, body, n_hist, L, M, n_out):
    """The filter over history + x from rest (everything in front of the history is zero), the history's outputs dropped."""
    xw = body.astype(np.complex128 if np.iscomplexobj(b) else _wide(body.dtype))
    if L > 1:
        up = np.zeros(xw.size * L, dtype=xw.dtype)
        up[::L] = L * xw
    else:
        up = xw
    return signal.lfilter(b, [1], up)[n_hist * L:][::M][:n_out]


def _fir_call(k, c, n_hist):
    L, M = c["L"], c["M"]
    if c["mode"] == "filter":
        return lambda xw, yw: k.filter_dev(xw, yw, n_hist=n_hist)
    if c["mode"] == "up":
        return lambda xw, yw: k.up_dev(xw, yw, L, n_hist=n_hist)
    if c["mode"] == "dn":
        return lambda xw, yw: k.dn_dev(xw, yw, M, n_hist=n_hist)
    return lambda xw, yw: k.updn_dev(xw, yw, L, M, n_hist=n_hist)


@pytest.mark.parametrize("case", FIR_CASES, ids=[c["name"] for c in FIR_CASES])
def test_fir_calls_read_their_window_only(case):
    c = case
    assert c["mode"] != "dn" or c["n"] % c["M"], "a .dn case must drop trailing samples"
    b = _taps(c)
    k = _ffi.FirKernel(b, _ffi.code_of(c["dt"]))
    n_out = _fir_n_out(c)
    for kind in c["hists"]:
        n_hist = _hist_len(c, kind)
        body = _noise(100 + n_hist, n_hist + c["n"], c["dt"])
        ref = _fir_ref(b, body, n_hist, c["L"], c["M"], n_out)
        bound = float(np.sum(np.abs(b)) * c["L"] * np.max(np.abs(body)))
        with _options(c["opts"]):
            footprint("fir %s %s" % (c["name"], np.dtype(c["dt"]).name), c["engine"], body, n_hist, n_out, _fir_call(k, c, n_hist), ref,
                      _tol(c["dt"]), bound=bound)


def touched(n_out, ntaps, L, M, ks):
    """Outputs that multiply x[k] for some k in ks: high-rate indices [k L, k L + Ntaps), every M-th kept (as tests/test_gpu_nonfinite.py)."""
    t = np.zeros(n_out, bool)
    for k in ks:
        lo, hi = k * L, k * L + ntaps
        t[max(-(-lo // M), 0):min(-(-hi // M), n_out)] = True
    return t


RECOMPUTE = ["ols_c64", "bx_f32", "up3_4k_c64_g4", "dn3_4k_c64", "ols64_f64"]


@pytest.mark.parametrize("name", RECOMPUTE)
def test_recompute_path_reads_its_window_only(name):
    """A NaN at x[0] and at x[n-1] INSIDE the window sends the first and the last tile / window through the non-finite recompute path
    (csrc/careful.hpp), which has loaders and guards of its own: loud pads must not change a byte, and outside the Ntaps outputs each NaN
    touches the result is finite and within the contract."""
    c = next(c for c in FIR_CASES if c["name"] == name)
    b = _taps(c)
    k = _ffi.FirKernel(b, _ffi.code_of(c["dt"]))
    n, L, M = c["n"], c["L"], c["M"]
    n_out = _fir_n_out(c)
    body = _noise(7, n, c["dt"])
    clean = body.copy()
    clean[[0, n - 1]] = 0        # (the outputs that never multiply the two samples are those of the signal without them)
    body[[0, n - 1]] = np.nan
    ref = _fir_ref(b, clean, 0, L, M, n_out)
    hit = touched(n_out, c["ntaps"], L, M, [0, n - 1])
    assert hit.any() and not hit.all()
    peak = float(np.max(np.abs(ref[~hit])))

    def check(y, path):
        assert np.all(np.isfinite(y[~hit])), "%s (%s): %d outputs that never see a NaN are not finite" % (name, path, int(np.sum(~np.isfinite(y[~hit]))))
        assert not np.any(np.isfinite(y[hit])), "%s: an output that multiplies a NaN came out finite" % name
        err = float(np.max(np.abs(y[~hit] - ref[~hit]))) / peak
        assert err <= _tol(c["dt"]), "%s (%s): error %.3g outside the outputs the NaNs touch, contract %.1g" % (name, path, err, _tol(c["dt"]))
        return err

    with _options(c["opts"]):
        footprint("recompute %s" % name, c["engine"], body, 0, n_out, _fir_call(k, c, 0), None, _tol(c["dt"]), fills=("zeros", "loud"), check=check)


# ---- rows
def _rows_layout(n, rows, x_stride, y_stride):
    nb, n_y = (rows - 1) * x_stride + n, (rows - 1) * y_stride + n
    return nb, n_y, (np.arange(nb) % x_stride) >= n, (np.arange(n_y) % y_stride) < n


@pytest.mark.parametrize("dt,ntaps,engine", [(F32, 127, "fir_bx"), (C64, 127, "fir_bx"), (C64, 1024, "fir_ols"), (F64, 48, "fir_mm")],
                         ids=["f32_127", "c64_127", "c64_1024", "f64_48"])
def test_fir_rows_read_their_rows_only(dt, ntaps, engine):
    """filter_rows_dev with x_stride > n: the gaps between the rows are filled like the pads; the gaps of y keep their sentinel."""
    n, rows, x_stride, y_stride = 5001, 3, 5001 + 37, 5001 + 5
    nb, n_y, gaps, written = _rows_layout(n, rows, x_stride, y_stride)
    b = signal.firwin(ntaps, 0.3)
    k = _ffi.FirKernel(b, _ffi.code_of(dt))
    body = _noise(31, nb, dt)
    ref = np.concatenate([signal.lfilter(b, [1], body[r * x_stride:r * x_stride + n].astype(_wide(dt))) for r in range(rows)])
    footprint("fir rows %s %d taps" % (np.dtype(dt).name, ntaps), engine, body, 0, n_y,
              lambda xw, yw: k.filter_rows_dev(xw, yw, n, rows, x_stride, y_stride), ref, _tol(dt), outside=gaps, y_written=written,
              bound=float(np.sum(np.abs(b)) * np.max(np.abs(body))))


# ================================================================================================================== IIR
def _sos8():
    return np.load(os.path.join(GOLDEN, "g7_iir_sos.npz"))["sos8"]    # an 8-biquad elliptic band-pass


def _v32_design(name="eq8lin(+12,Q2)"):
    z = np.load(os.path.join(GOLDEN, "g18_v32_designs.npz"))
    i = [str(s) for s in z["names"]].index(name)
    return z["sos"][i, :z["nsec"][i]].copy()


def _rc12():
    rc = mrh.rate_change(12)
    return dict(b=rc.b, a=rc.a)


def _iir(name, engine, dts, design, mode="filter", f=1, opts=None, n=20001, absent=(), exact=False):
    return dict(name=name, engine=engine, dts=dts, design=design, mode=mode, f=f, opts=opts or {}, n=n, absent=absent, exact=exact)


ALL4 = (F32, C64, F64, C128)
SCANS = {"iir_par": 0}
IIR_CASES = [
    _iir("par_ellip8", "iir_par", ALL4, _sos8),
    _iir("cascade_ellip8", "iir_scan", ALL4, _sos8, opts=SCANS, absent=("iir_par",)),
    _iir("two_pass_ellip8", "iir_scan", ALL4, _sos8, opts=dict(SCANS, iir_two_pass=1), absent=("iir_par", "iir_fused")),
    _iir("groups_butter24", ("iir_scan", "iir_par"), ALL4, lambda: signal.butter(24, 0.2, output="sos"), absent=("iir_seq",)),
    _iir("seq_cheby40", "iir_seq", (F64,), lambda: signal.cheby1(40, 0.5, 0.3, output="sos"), exact=True),
    _iir("v32_eq8", "iir_par_v32", (F32, C64), _v32_design, opts={"iir_par_v32": 2}),
    _iir("up2_ellip8", "iir_par", ALL4, _sos8, mode="up", f=2, n=12289),
    _iir("up12_ellip8", "iir_par", ALL4, _sos8, mode="up", f=12, n=12289),
    _iir("dn3_ellip8", "iir_par", ALL4, _sos8, mode="dn", f=3, n=20003),
    _iir("dn12_ellip8", "iir_par", ALL4, _sos8, mode="dn", f=12, n=20003),
    _iir("dn12_rate_change", "iir_par", ALL4, _rc12, mode="dn", f=12, n=20003),           # (order-8 Butterworth: the lean forms)
    _iir("dn3_cascade", "iir_scan", (F32, C64), _sos8, mode="dn", f=3, n=20003, opts=SCANS, absent=("iir_par",)),
]


def _iir_design(c):
    d = c["design"]()
    if isinstance(d, dict):   # a transfer function: the reference is its float64 cascade, as far as (b, a) itself holds it
        sos = signal.tf2sos(d["b"], d["a"])
        return d, sos
    return dict(sos=d), d


def _iir_ref(sos, tf, x, mode, f):
    xw = x.astype(_wide(x.dtype))
    if mode == "up":
        up = np.zeros(xw.size * f, dtype=xw.dtype)
        up[::f] = f * xw
        xw = up
    ref = signal.sosfilt(sos, xw)
    spread = 0.0
    if "b" in tf:       # two float64 evaluations of the same filter: what the reference itself is good to (test_gpu_fuzz)
        spread = float(np.max(np.abs(ref - signal.lfilter(tf["b"], tf["a"], xw))))
    elif len(sos) > 8:
        spread = float(np.max(np.abs(ref - signal.sosfilt(np.ascontiguousarray(sos[::-1]), xw))))
    if mode == "dn":
        ref = ref[::f][:x.size // f]
    return ref, spread


@pytest.mark.parametrize("case", IIR_CASES, ids=[c["name"] for c in IIR_CASES])
def test_iir_calls_read_their_window_only(case):
    c = case
    tf, sos = _iir_design(c)
    h = signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)])
    for dt in c["dts"]:
        k = _ffi.IirKernel(_ffi.code_of(dt), **tf)
        n, mode, f = c["n"], c["mode"], c["f"]
        assert mode != "dn" or n % f
        x = _noise(200 + f, n, dt)
        ref, spread = _iir_ref(sos, tf, x, mode, f)
        if c["exact"]:
            ref = ref.astype(dt)
        n_y = ref.size
        call = {"filter": lambda xw, yw: k.filter_dev(xw, yw), "up": lambda xw, yw: k.up_dev(xw, yw, f),
                "dn": lambda xw, yw: k.dn_dev(xw, yw, f)}[mode]
        bound = float(np.sum(np.abs(h)) * np.max(np.abs(x))) * (f if mode == "up" else 1)
        what = "iir %s %s" % (c["name"], np.dtype(dt).name)

        def check(y, path, ref=ref, spread=spread, dt=dt, bound=bound, what=what):
            assert not set(path) & set(c["absent"]), (what, path)
            scale = max(float(np.max(np.abs(ref))), 1e-2 * bound)
            err = float(np.max(np.abs(y - ref)))
            assert err <= _tol(dt) * scale + 30.0 * spread, "%s: err %.3g, scale %.3g, reference spread %.3g" % (what, err, scale, spread)
            return err / scale   # (reported; the assertion above is the contract, test_gpu_fuzz._check's)

        with _options(c["opts"]):
            footprint(what, c["engine"], x, 0, n_y, call, ref, _tol(dt), bound=bound, exact=c["exact"], check=None if c["exact"] else check)


def _lowpass4():
    return signal.ellip(8, 0.5, 60, 0.3, output="sos")


# (dtype, samples per chunk, cascade): the scan is admitted where the cascade's transition over one segment of 256 chunks has vanished
# (below 1e-18 for float32 / complex64, 1e-30 for float64 / complex128): the 8-biquad band-pass (largest pole radius 0.99465) everywhere
# but on complex128's 32-sample chunks (0.99465^8192 = 8e-20), which take a 4-biquad elliptic low-pass (radius 0.98536)
SINGLE_PASS = [(F32, 128, _sos8), (C64, 64, _sos8), (F64, 64, _sos8), (C128, 32, _lowpass4)]


@pytest.mark.parametrize("dt,chunk,design", SINGLE_PASS, ids=[np.dtype(c[0]).name for c in SINGLE_PASS])
def test_iir_single_pass_scan_reads_its_window_only(dt, chunk, design):
    """The single-pass scan (iir_fused.hip; real signals and, a kernel of its own, interleaved complex ones) takes a call only from one chunk
    per thread of the whole device on (128 float32 / 64 float64 / 64 complex64 / 32 complex128 samples x 256 threads x the compute units):
    the smallest such signal, ragged by 77 samples."""
    _ffi.init()
    n = chunk * 256 * _ffi.device_info()["compute_units"] + 77
    sos = design()
    k = _ffi.IirKernel(_ffi.code_of(dt), sos=sos)
    x = _noise(9, n, dt)
    ref = signal.sosfilt(sos, x.astype(_wide(dt)))
    with _options(dict(SCANS, iir_two_pass=-1)):
        footprint("iir single pass %s" % np.dtype(dt).name, "iir_fused", x, 0, n, lambda xw, yw: k.filter_dev(xw, yw), ref, _tol(dt))


@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_iir_state_call_reads_its_window_only(dt):
    """filter_state_dev behind a non-zero zi: the output and the returned zf."""
    sos = _sos8()
    k = _ffi.IirKernel(_ffi.code_of(dt), sos=sos)
    n = 20001
    x = _noise(12, n, dt)
    zi = np.random.default_rng(13).standard_normal((len(sos), 2)) * 0.1
    ref, zf_ref = signal.sosfilt(sos, x.astype(np.float64), zi=zi)
    zfs = []

    def call(xw, yw):
        zfs.append(k.filter_state_dev(xw, yw, zi=zi.ravel()))
        return zfs[-1]

    footprint("iir state %s" % np.dtype(dt).name, "iir_scan", x, 0, n, call, ref, _tol(dt))
    e = float(np.max(np.abs(zfs[0].reshape(-1, 2) - zf_ref)) / np.max(np.abs(zf_ref)))
    print("iir state %s: zf error %.3g" % (np.dtype(dt).name, e))
    assert e <= _tol(dt)


@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
@pytest.mark.parametrize("design", ["ellip8", "butter24"])
def test_iir_rows_read_their_rows_only(design, dt):
    n, rows, x_stride, y_stride = 5001, 3, 5001 + 37, 5001 + 5
    nb, n_y, gaps, written = _rows_layout(n, rows, x_stride, y_stride)
    sos = _sos8() if design == "ellip8" else signal.butter(24, 0.2, output="sos")
    k = _ffi.IirKernel(_ffi.code_of(dt), sos=sos)
    body = _noise(41, nb, dt)
    rows_x = [body[r * x_stride:r * x_stride + n].astype(np.float64) for r in range(rows)]
    ref = np.concatenate([signal.sosfilt(sos, v) for v in rows_x])
    spread = 0.0 if len(sos) <= 8 else max(float(np.max(np.abs(signal.sosfilt(sos, v) - signal.sosfilt(np.ascontiguousarray(sos[::-1]), v)))) for v in rows_x)
    peak = float(np.max(np.abs(ref)))

    def check(y, path):
        err = float(np.max(np.abs(y - ref)))
        assert err <= _tol(dt) * peak + 30.0 * spread, (design, err, peak, spread)
        return err / peak

    footprint("iir rows %s %s" % (design, np.dtype(dt).name), "iir_par" if design == "ellip8" else ("iir_scan", "iir_par"), body, 0, n_y,
              lambda xw, yw: k.filter_rows_dev(xw, yw, n, rows, x_stride, y_stride), ref, _tol(dt), outside=gaps, y_written=written, check=check)


# ================================================================================================== the other device entry points
@pytest.mark.parametrize("dt", [C64, F64], ids=["complex64", "float64"])
@pytest.mark.parametrize("fs_old,fs_new", [(48000, 44100), (20, 1)], ids=["48000_44100", "20_1"])
def test_farrow_reads_its_window_only(fs_old, fs_new, dt):
    n = 20001
    x = _noise(51, n, dt)
    count = _ffi.farrow_len(n, 1 / fs_old, 1 / fs_new)
    ref = farrow_restated(x, fs_old, fs_new, 3)
    assert ref.size == count
    footprint("farrow %d -> %d %s" % (fs_old, fs_new, np.dtype(dt).name), "farrow", x, 0, count,
              lambda xw, yw: _ffi.farrow_dev(xw, yw, 1 / fs_old, 1 / fs_new, 3, 0.5), ref, _tol(dt))


PSD_CASES = [(256, 200, 77, 150), (256, 256, 77, 200), (1024, 1024, 512, 24)]   # (n_fft, window length ns, step, segments)


@pytest.mark.parametrize("dt", ALL4, ids=[np.dtype(d).name for d in ALL4])
@pytest.mark.parametrize("n_fft,ns,step,nseg", PSD_CASES, ids=["256_ns200_step77", "256_step77", "1024_half"])
def test_psd_reads_its_window_only(n_fft, ns, step, nseg, dt):
    """The Welch primitive: the first segment begins at the window's first sample, the last one ends at its last.  ns < n_fft (a 200-sample
    window zero-padded into a 256-point transform): the transform's last n_fft - ns inputs of the last segment would lie in the back pad."""
    n = (nseg - 1) * step + ns
    x = _noise(61, n, dt)
    w = signal.windows.hann(ns)
    ref = ss.psd_accum_host(x, w, n_fft, step, nseg)
    footprint("psd %d/%d/%d/%d %s" % (n_fft, ns, step, nseg, np.dtype(dt).name), "psd", x, 0, n_fft,
              lambda xw, yw: _ffi.psd_accum_dev(xw, yw, w, n_fft, step, nseg), ref, _tol(dt), y_dtype=np.float64)


@pytest.mark.parametrize("dt", [C64, F32], ids=["complex64", "float32"])
def test_fir_bank_reads_its_window_only(dt):
    n, stride, shifts, period = 12289, 12289 + 11, [-3, 0, 5], 2000
    g = signal.firwin(96, 0.3) * np.exp(0.2j * np.arange(96))
    bank = _ffi.FirBank(g, shifts, period, dt)
    x = _noise(71, n, dt)
    ref = np.concatenate([signal.lfilter(ss._caf_band_taps(g, s, period), 1.0, x.astype(np.complex128)) for s in shifts])
    n_y = (len(shifts) - 1) * stride + n
    footprint("fir bank %s" % np.dtype(dt).name, "fir_bank4k", x, 0, n_y, lambda xw, yw: bank.filter_dev(xw, yw, stride), ref, 1e-6,
              y_dtype=np.complex64, y_written=(np.arange(n_y) % stride) < n)


@pytest.mark.parametrize("dt", ALL4, ids=[np.dtype(d).name for d in ALL4])
def test_resampling_copies_read_their_window_only(dt):
    """skdsp_upsample_dev / skdsp_downsample_dev (the device forms of sigsys.upsample / downsample): bit-exact copies.  These calls
    note no engine (skdsp_debug_path stays empty), so there is none to assert: the path must only be the same for every fill."""
    lib = _ffi.load()
    code = _ffi.code_of(dt)
    n = 12289
    x = _noise(81, n, dt)
    for L in (3, 12):
        ref = np.zeros(n * L, dtype=dt)
        ref[::L] = x
        footprint("upsample by %d %s" % (L, np.dtype(dt).name), None, x, 0, n * L,
                  lambda xw, yw: _ffi.check(lib.skdsp_upsample_dev(ctypes.c_void_p(xw.ptr), n, L, code, 1.0, ctypes.c_void_p(yw.ptr))), ref, 0.0, exact=True)
    for M, p in ((3, 1), (12, 11)):
        assert n % M
        ref = x[p::M][:n // M]
        footprint("downsample by %d phase %d %s" % (M, p, np.dtype(dt).name), None, x, 0, n // M,
                  lambda xw, yw: _ffi.check(lib.skdsp_downsample_dev(ctypes.c_void_p(xw.ptr), n, M, p, code, ctypes.c_void_p(yw.ptr))), ref, 0.0, exact=True)
