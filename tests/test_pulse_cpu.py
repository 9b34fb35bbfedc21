"""Pulse shaping and matched filtering over frame sets without a GPU: the NumPy host forms against results captured from the real reference
(tests/golden/gen_golden_pulse.py -> g26_pulse.npz, g26_conventions.json), and both kernels walked thread by thread on the CPU
(tests/host/pulse_emul.cpp) with every global and LDS access bounds-checked, once more under -fsanitize=address,undefined as a stand-alone
program.  DESIGN.md 4.21.

The bound against the reference.  The reference's lfilter (a = 1) runs np.convolve, whose summation order is the dot product's; the host forms
and the kernels add the terms of an output from the oldest sample to the newest.  Both orders lie within J u sum|b| max|s| of the exact sum of J
products (u = 2^-53), the scale and the complex combination add one rounding each: (2 J + 2) u sum|b| max|s| |c|, absolute, per output.  Between
the host forms, the emulation and the device the comparison is array_equal."""
import json
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc, sigsys as ss
from conftest import ROOT

U = 2.0 ** -53
CODES = {np.dtype(np.float32): 0, np.dtype(np.complex64): 1, np.dtype(np.float64): 2, np.dtype(np.complex128): 3}
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
G = np.load(os.path.join(ROOT, "tests", "golden", "g26_pulse.npz"))
CONV = json.load(open(os.path.join(ROOT, "tests", "golden", "g26_conventions.json")))
ENC, MF, NRZ = (json.loads(str(G[k])) for k in ("enc", "mf", "nrz"))
ENCODERS = {"qam": (dc.qam_gray_encode_bb_rows_host, _ffi.QAM), "mpsk": (dc.mpsk_gray_encode_bb_rows_host, _ffi.MPSK)}


def order_bound(ntaps, ns, n, b, smax, c=1.0):
    """(2 J + 2) u sum|b| max|s| |c| per output of a shaped row: J = the taps of the output's phase"""
    J = np.array([len(range(p, ntaps, ns)) for p in range(ns)], dtype=np.float64)
    return np.tile((2 * J + 2) * U * np.sum(np.abs(b)) * smax * abs(c), n)


def worst(err, bound):
    return float(np.max(err / bound)) if err.size else 0.0


def signal_of(rng, shape, dt):
    x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if np.dtype(dt).kind == "c" else 0)
    return x.astype(dt)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def test_fixture_covers_what_the_issue_lists():
    assert {(c["kind"], c["mod"]) for c in ENC} == {("qam", m) for m in (2, 4, 16, 256)} | {("mpsk", m) for m in (2, 8, 32)}
    assert {(c["ns"], c["pulse"]) for c in ENC} == {(ns, p) for ns in (1, 2, 3, 8, 16) for p in ("rect", "rc", "src")}
    assert {(c["pulse"], c["m_span"]) for c in ENC} >= {(p, m) for p in ("rc", "src") for m in (2, 6)}
    assert max(c["n_symb"] for c in ENC) <= 300 and all(G[c["key"] + "_x"].size == c["n_symb"] * c["ns"] for c in ENC)
    assert all(set(c["starts"]) == {0, 5, 2 * c["m_span"] * c["ns"]} for c in MF) and {c["pulse"] for c in MF} == {"rect", "rc", "src"}
    assert {G[c["key"] + "_x"].dtype.kind for c in MF} == {"f", "c"} and len(NRZ) >= 4
    for obs in CONV["complex_array_divided_by_real_scalar"].values():
        assert obs["equals_component_times_reciprocal"] and not obs["equals_component_quotient"]
    assert CONV["numpy"] and CONV["scipy"]


def test_numpy_still_divides_a_complex_array_by_a_real_scalar_as_the_fixture_records():
    z = np.random.default_rng(26).standard_normal(2000) * (1 + 1j)
    for x_m in (3.0, 7.0, 15.0):
        assert np.array_equal((z / x_m).real, z.real * (1 / x_m)) and not np.array_equal((z / x_m).real, z.real / x_m)


# ---------------------------------------------------------------------------------------------------------------- host forms against the reference
@pytest.mark.parametrize("c", ENC, ids=[c["key"] for c in ENC])
def test_encoder_host_forms_meet_the_reference_within_the_order_bound(c):
    fn, kind = ENCODERS[c["kind"]]
    bits = G[c["key"] + "_bits"]
    x, b = fn(bits[None, :], c["ns"], c["mod"], c["pulse"], c["alpha"], c["m_span"])
    ref = G[c["key"] + "_x"]
    assert x.shape == (1, ref.size) and x.dtype == np.complex128
    if c["ns"] == 1:
        assert b == 1 and G[c["key"] + "_b"] == 1
        taps = np.ones(1)
    else:
        # (the package's rc_imp / sqrt_rc_imp, which the 1-D transmitters use too, lie up to 3.4e-16 from the reference's at ns = 3)
        assert b.shape == G[c["key"] + "_b"].shape and np.max(np.abs(b - G[c["key"] + "_b"])) <= 4 * U
        taps = ss._pulse(c["pulse"], c["ns"], c["alpha"], c["m_span"])
    (tre, tim), scale = _ffi.gray_levels(kind, c["mod"])
    sym = _ffi.gray_map_rows_host(bits[None, :], kind, c["mod"], table=(tre, tim))
    bound = order_bound(taps.size, c["ns"], c["n_symb"], taps, np.max(np.abs(sym)), 1.0 if scale is None else scale)
    err = np.maximum(np.abs(x[0].real - ref.real), np.abs(x[0].imag - np.imag(ref)))
    print("encoder", c["key"], c["kind"], c["mod"], c["ns"], c["pulse"], "worst error / bound = %.3f" % worst(err, bound))
    assert np.all(err <= bound)


@pytest.mark.parametrize("c", MF, ids=[c["key"] for c in MF])
def test_matched_filter_host_form_meets_lfilter_within_the_order_bound(c):
    x, b = G[c["key"] + "_x"], G[c["key"] + "_b"]
    comp = np.max(np.abs(x))
    for start in c["starts"]:
        z = ss.matched_filter_rows_host(x[None, :], b, start, c["ns"])
        ref = G[c["key"] + "_z%d" % start]
        assert z.shape == (1, ref.size) and z.dtype == x.dtype
        bound = (2 * b.size + 2) * U * np.sum(np.abs(b)) * comp
        err = np.maximum(np.abs(z[0].real - ref.real), np.abs(np.imag(z[0]) - np.imag(ref)))
        print("matched filter", c["key"], c["ns"], start, "worst error / bound = %.3f" % worst(err, np.full(err.shape, bound)))
        assert np.all(err <= bound)


@pytest.mark.parametrize("c", NRZ, ids=[c["key"] for c in NRZ])
def test_shaping_host_form_meets_nrz_bits2_within_the_order_bound(c):
    data = G[c["key"] + "_data"].astype(np.int64)
    taps = ss._pulse(c["pulse"], c["ns"], c["alpha"], c["m"])
    x = ss.pulse_shape_rows_host((2 * data - 1)[None, :], taps, c["ns"])
    ref = G[c["key"] + "_x"]
    assert x.dtype == np.float64 and x.shape == (1, ref.size) and np.array_equal(taps / float(c["ns"]), G[c["key"] + "_b"])
    bound = order_bound(taps.size, c["ns"], data.size, taps, 1.0)
    print("nrz_bits2", c["key"], "worst error / bound = %.3f" % worst(np.abs(x[0] - ref), bound))
    assert np.all(np.abs(x[0] - ref) <= bound)


# ---------------------------------------------------------------------------------------------------------------- the host forms themselves
def test_single_precision_results_are_the_double_result_rounded_once():
    rng = np.random.default_rng(2601)
    b = rng.standard_normal(23)
    for dt, wide in ((np.float32, np.float64), (np.complex64, np.complex128)):
        x = signal_of(rng, (3, 41), dt)
        y, y_wide = ss.pulse_shape_rows_host(x, b, 4, 1 / 7.0), ss.pulse_shape_rows_host(x.astype(wide), b, 4, 1 / 7.0)
        assert y.dtype == dt and y_wide.dtype == wide and np.array_equal(y, y_wide.astype(dt)) and not np.array_equal(y, y_wide)
        z, z_wide = ss.matched_filter_rows_host(x, b, 3, 4), ss.matched_filter_rows_host(x.astype(wide), b, 3, 4)
        assert z.dtype == dt and np.array_equal(z, z_wide.astype(dt)) and not np.array_equal(z, z_wide)


def test_rows_are_independent_frames_and_equal_the_one_row_result():
    rng = np.random.default_rng(2602)
    b = rng.standard_normal(29)
    x = signal_of(rng, (4, 37), np.complex128)
    y, z = ss.pulse_shape_rows_host(x, b, 3, -0.5), ss.matched_filter_rows_host(x, b, 5, 3)
    for r in range(4):
        assert np.array_equal(y[r], ss.pulse_shape_rows_host(x[r:r + 1], b, 3, -0.5)[0]) and np.array_equal(z[r], ss.matched_filter_rows_host(x[r:r + 1], b, 5, 3)[0])
    bits = rng.integers(0, 2, (3, 96)).astype(np.uint8)
    for fn, mod in ((dc.qam_gray_encode_bb_rows_host, 16), (dc.mpsk_gray_encode_bb_rows_host, 8)):
        x2, b2 = fn(bits, 8, mod, 'src', 0.35, 6, np.complex64)
        assert x2.dtype == np.complex64 and b2.size == 97
        for r in range(3):
            assert np.array_equal(x2[r], fn(bits[r:r + 1], 8, mod, 'src', 0.35, 6, np.complex64)[0][0])
    # shaping is lfilter of the stuffed row, the matched filter lfilter read at start::step: a brute-force double loop in the kernel's order
    s, taps = signal_of(rng, (1, 9), np.float64), rng.standard_normal(7)
    want = np.zeros(27)
    for o in range(27):
        k, p = divmod(o, 3)
        for j in range((7 - 1 - p) // 3, -1, -1):
            want[o] = taps[p + 3 * j] * (s[0, k - j] if k - j >= 0 else 0.0) + want[o]
    assert np.array_equal(ss.pulse_shape_rows_host(s, taps, 3)[0], want)
    want = np.zeros(3)
    for k in range(3):
        for i in range(6, -1, -1):
            g = 2 + 3 * k - i
            want[k] = taps[i] * (s[0, g] if g >= 0 else 0.0) + want[k]
    assert np.array_equal(ss.matched_filter_rows_host(s, taps, 2, 3)[0], want)


def test_argument_errors_need_no_device():
    x, b = np.ones((2, 8)), np.ones(5)
    for fn in (ss.pulse_shape_rows, ss.pulse_shape_rows_host):
        with pytest.raises(ValueError, match="2-D"):
            fn(np.ones(8), b, 2)
        with pytest.raises(ValueError, match="ns"):
            fn(x, b, 0)
        with pytest.raises(ValueError, match="ns"):
            fn(x, b, 2.5)
        with pytest.raises(ValueError, match="tap"):
            fn(x, np.ones((2, 2)), 2)
        with pytest.raises(TypeError):
            fn(np.array([["a"]]), b, 2)
    for fn in (ss.matched_filter_rows, ss.matched_filter_rows_host):
        with pytest.raises(ValueError, match="2-D"):
            fn(np.ones(8), b)
        with pytest.raises(ValueError, match="step"):
            fn(x, b, 0, 0)
        with pytest.raises(ValueError, match="start"):
            fn(x, b, -1, 2)
        with pytest.raises(ValueError, match="tap"):
            fn(x, np.zeros(0), 0, 1)
    assert ss.matched_filter_rows(x, b, 8, 2).shape == (2, 0) and ss.matched_filter_rows(x, b, 11, 1).shape == (2, 0)      # empty outputs launch nothing
    assert ss.pulse_shape_rows(np.zeros((0, 4)), b, 3).shape == (0, 12) and ss.pulse_shape_rows(np.zeros((2, 0), dtype=np.complex64), b, 3).dtype == np.complex64
    bits = np.zeros((2, 8), dtype=np.uint8)
    for fn in (dc.qam_gray_encode_bb_rows, dc.qam_gray_encode_bb_rows_host):
        with pytest.raises(ValueError, match="M must be 2, 4, 16, 64, 256"):
            fn(bits, 4, 8)
        with pytest.raises(ValueError, match="pulse shape must be src, rc, or rect"):
            fn(bits, 4, 4, 'gauss')
        with pytest.raises(ValueError, match="bits 0 / 1"):
            fn(bits + 2, 4, 4)
        with pytest.raises(TypeError, match="complex64 or complex128"):
            fn(bits, 4, 4, dtype=np.float64)
    for fn in (dc.mpsk_gray_encode_bb_rows, dc.mpsk_gray_encode_bb_rows_host):
        with pytest.raises(ValueError, match="M must be 2, 4, 8, 16, or 32"):
            fn(bits, 4, 64)
        with pytest.raises(ValueError, match="pulse shape must be src, rc, or rect"):
            fn(bits, 4, 4, 'gauss')
        with pytest.raises(ValueError, match="2-D"):
            fn(bits[0], 4, 4)


def test_c_abi_argument_rules_need_no_device():
    L = _ffi.load()
    k = _ffi.PulseKernel(np.ones(5), np.complex64)
    shape = lambda n, nrow, xs, ns, ys: L.skdsp_pulse_shape_rows_dev(k.h, None, n, nrow, xs, ns, None, None, ys)
    mf = lambda n, nrow, xs, start, step, ys: L.skdsp_pulse_mf_rows_dev(k.h, None, n, nrow, xs, start, step, None, ys)
    assert shape(0, 2, 0, 4, 0) == 0 and shape(10, 0, 10, 4, 40) == 0 and mf(10, 0, 10, 0, 2, 5) == 0 and mf(10, 2, 10, 10, 2, 0) == 0 and mf(10, 2, 10, 13, 1, 0) == 0
    assert shape(10, 2, 10, 4, 39) == -1 and b"y_stride" in L.skdsp_last_error()
    assert shape(10, 2, 9, 4, 40) == -1 and b"x_stride" in L.skdsp_last_error()
    assert shape(10, 2, 10, 0, 40) == -1 and shape(-1, 2, 10, 4, 40) == -1 and shape(10, -2, 10, 4, 40) == -1
    assert shape(10, 2, 10, 65, 650) == -6 and shape(10, 2, 10, 64, 640) == -1 and b"null pointer" in L.skdsp_last_error()
    assert mf(10, 2, 10, 0, 3, 3) == -1 and b"y_stride" in L.skdsp_last_error() and mf(10, 2, 10, 0, 3, 4) == -1 and b"null pointer" in L.skdsp_last_error()
    assert mf(10, 2, 9, 0, 3, 4) == -1 and mf(10, 2, 10, -1, 3, 4) == -1 and mf(10, 2, 10, 0, 0, 10) == -1 and mf(10, 2, 10, 0, 65, 1) == -6
    y = np.zeros(80, dtype=np.complex64)
    assert L.skdsp_pulse_shape_rows(k.h, None, 10, 2, 65, None, _ffi._ptr(y)) == -6 and L.skdsp_pulse_mf_rows(k.h, None, 10, 2, 0, 65, _ffi._ptr(y)) == -6
    assert L.skdsp_pulse_shape_rows(k.h, None, 0, 2, 4, None, None) == 0 and L.skdsp_pulse_mf_rows(k.h, None, 10, 2, 10, 3, None) == 0
    h = _ffi.ctypes.c_void_p(0)
    taps = np.ones(2050)
    assert L.skdsp_pulse_create(_ffi._ptr(taps), 2050, 1, _ffi.ctypes.byref(h)) == -6 and L.skdsp_pulse_create(_ffi._ptr(taps), 0, 1, _ffi.ctypes.byref(h)) == -1
    assert L.skdsp_pulse_create(_ffi._ptr(taps), 5, 7, _ffi.ctypes.byref(h)) == -1 and L.skdsp_pulse_create(None, 5, 1, _ffi.ctypes.byref(h)) == -1
    fir = _ffi.ConvCodeKernel(('111', '101'))
    assert L.skdsp_pulse_shape_rows_dev(fir.h, None, 10, 2, 10, 4, None, None, 40) == -1 and b"not a pulse handle" in L.skdsp_last_error()
    assert _ffi.PulseKernel.mf_out_len(10, 0, 3) == 4 and _ffi.PulseKernel.mf_out_len(10, 9, 64) == 1 and _ffi.PulseKernel.mf_out_len(10, 10, 1) == 0
    with pytest.raises(TypeError, match="complex64"):
        k.shape_rows(np.ones((1, 4)), 2)


def test_the_built_library_exports_the_new_symbols():
    L = _ffi.load()
    names = ["skdsp_pulse_create", "skdsp_pulse_mf_out_len", "skdsp_pulse_shape_rows", "skdsp_pulse_shape_rows_dev", "skdsp_pulse_mf_rows", "skdsp_pulse_mf_rows_dev"]
    assert all(n in _ffi.SYMBOLS and hasattr(L, n) for n in names)
    header = open(os.path.join(ROOT, "include", "skdsp.h")).read()
    assert all(("int %s(" % n) in header for n in names)


# ---------------------------------------------------------------------------------------------------------------- the emulation
def build_emul(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "pulse_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("pulse"), "pulse_emul", [])


def words(exe, *args):
    return [int(w) for w in subprocess.check_output([exe] + [str(a) for a in args]).decode().split()]


def plan_of(exe):
    return dict(zip(("threads", "shape_out", "mf_in", "max_taps", "max_rate"), words(exe, "plan")))


def shape_plan(exe, dt, ntaps, ns, n):
    return dict(zip(("J", "H", "T", "tiles", "lds"), words(exe, "shapeplan", CODES[np.dtype(dt)], ntaps, ns, n)))


def mf_plan(exe, dt, ntaps, n, start, step, naive=0):
    return dict(zip(("R", "To", "W", "Wq", "tiles", "lds", "n_out"), words(exe, "mfplan", CODES[np.dtype(dt)], ntaps, n, start, step, naive)))


def strided(x, stride):
    """the rows of x laid `stride` elements apart, through the last row's last element (what a call may read)"""
    nrow, n = x.shape
    flat = np.zeros(((nrow - 1) * stride + n) if nrow and n else 0, dtype=x.dtype)
    for r in range(nrow):
        flat[r * stride:r * stride + n] = x[r]
    return flat


def emul_shape(exe, tmp, x, b, ns, scale=None, x_stride=None, y_stride=None):
    nrow, n = x.shape
    xs, ys = n if x_stride is None else x_stride, n * ns if y_stride is None else y_stride
    fb, fx, fy = (os.path.join(str(tmp), f) for f in ("b.bin", "x.bin", "y.bin"))
    np.ascontiguousarray(b, dtype=np.float64).tofile(fb)
    strided(x, xs).tofile(fx)
    subprocess.check_call([exe, "shape", str(CODES[x.dtype]), str(b.size), str(ns), str(n), str(nrow), str(xs), str(ys), "0" if scale is None else "1",
                           float(1.0 if scale is None else scale).hex(), fb, fx, fy])
    return gaps_checked(open(fy, "rb").read(), x.dtype, nrow, n * ns, ys)


def emul_mf(exe, tmp, x, b, start, step, x_stride=None, y_stride=None, naive=0, fma=0):
    nrow, n = x.shape
    n_out = _ffi.sym_count(n, start, step)
    xs, ys = n if x_stride is None else x_stride, n_out if y_stride is None else y_stride
    fb, fx, fy = (os.path.join(str(tmp), f) for f in ("b.bin", "x.bin", "y.bin"))
    np.ascontiguousarray(b, dtype=np.float64).tofile(fb)
    strided(x, xs).tofile(fx)
    subprocess.check_call([exe, "mf", str(CODES[x.dtype]), str(b.size), str(n), str(nrow), str(start), str(step), str(xs), str(ys), str(naive), str(fma), fb, fx, fy])
    raw = open(fy, "rb").read()
    if n_out == 0:
        assert raw == b""
        return np.zeros((nrow, 0), dtype=x.dtype)
    return gaps_checked(raw, x.dtype, nrow, n_out, ys)


def gaps_checked(raw, dt, nrow, n_out, stride):
    """the rows of an output block; the bytes between the rows must still hold the fill"""
    esz = np.dtype(dt).itemsize
    assert len(raw) == ((nrow - 1) * stride + n_out) * esz
    buf = np.frombuffer(raw, dtype=np.uint8)
    for r in range(nrow - 1):
        assert np.all(buf[(r * stride + n_out) * esz:(r + 1) * stride * esz] == 0xA5), "a gap between two output rows was written"
    flat = np.frombuffer(raw, dtype=dt)
    return np.stack([flat[r * stride:r * stride + n_out] for r in range(nrow)])


NS_SET = (1, 3, 8, 64)


def taps_set(ns):
    return sorted({1, ns, 7, 2049})


def test_plans_are_functions_of_the_sizes(emul):
    P = plan_of(emul)
    assert P == dict(threads=256, shape_out=2048, mf_in=4096, max_taps=_ffi.PULSE_MAX_TAPS, max_rate=_ffi.PULSE_MAX_RATE)
    for ns in NS_SET + (2, 5, 63):
        for ntaps in taps_set(ns):
            p = shape_plan(emul, np.complex128, ntaps, ns, 10 ** 6)
            assert p["T"] == P["shape_out"] // ns and p["J"] == -(-ntaps // ns) and p["H"] == p["J"] - 1 and p["tiles"] == -(-10 ** 6 // p["T"])
            assert p["lds"] == ntaps + 2 * (p["T"] + p["H"]) and shape_plan(emul, np.float32, ntaps, ns, 7)["lds"] == ntaps + p["T"] + p["H"]
            assert p["lds"] * 8 <= 160 * 1024
    for step in NS_SET + (2, 4, 5, 9, 16, 17, 32):
        for ntaps in taps_set(step):
            p = mf_plan(emul, np.complex128, ntaps, 10 ** 6, 5, step)
            assert p["R"] == (4 if step <= 4 else 2 if step <= 8 else 1) and p["To"] == min(256 * p["R"], P["mf_in"] // step) and p["W"] == (p["To"] - 1) * step + ntaps
            assert p["n_out"] == -(-(10 ** 6 - 5) // step) and p["tiles"] == -(-p["n_out"] // p["To"])
            assert p["Wq"] % 2 == 1 and p["W"] <= p["Wq"] * step <= p["W"] + 3 * step             # the phase planes hold the window
            even = ntaps + ntaps % 2
            assert p["lds"] == even + 2 * step * p["Wq"] and p["lds"] * 8 <= 160 * 1024
            assert mf_plan(emul, np.float64, ntaps, 10 ** 6, 5, step)["lds"] == even + step * p["Wq"]
            assert mf_plan(emul, np.complex128, ntaps, 10 ** 6, 5, step, naive=1)["lds"] == even + 2 * p["W"]


def test_emulated_shaping_kernel_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(2603)
    i = 0
    for ns in NS_SET:
        for ntaps in taps_set(ns):
            p = shape_plan(emul, np.complex128, ntaps, ns, 1)
            sizes = sorted({1, max(1, p["J"] - 1), p["T"] - 1, p["T"], p["T"] + 1, 2 * p["T"] + 3} - {0})
            for n in sizes:
                dt, nrow = DTYPES[i % 4], (1, 3)[i % 2]
                scale = (None, 1 / 3.0, -1 / 15.0)[i % 3]
                xs, ys = n + (0, 5)[(i // 2) % 2], n * ns + (0, 3)[(i // 3) % 2]
                x, b = signal_of(rng, (nrow, n), dt), rng.standard_normal(ntaps)
                got = emul_shape(emul, tmp_path, x, b, ns, scale, xs, ys)
                assert np.array_equal(got, ss.pulse_shape_rows_host(x, b, ns, scale)), (ns, ntaps, n, dt)
                i += 1
    assert i >= 60


def test_emulated_matched_filter_kernel_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(2604)
    i = 0
    for step in NS_SET:
        for ntaps in taps_set(step):
            To = mf_plan(emul, np.complex128, ntaps, 1, 0, step)["To"]
            for k in sorted({1, max(1, -(-ntaps // step) - 1), To - 1, To, To + 1, 2 * To + 3}):      # outputs of a row
                dt, nrow, start = DTYPES[i % 4], (1, 3)[i % 2], (0, 5)[(i // 2) % 2]
                n = start + (k - 1) * step + 1 + (i % 3 if step > 2 else 0)                             # (a tail that adds no output)
                assert _ffi.sym_count(n, start, step) == k
                xs, ys = n + (0, 7)[(i // 2) % 2], k + (0, 2)[(i // 3) % 2]
                x, b = signal_of(rng, (nrow, n), dt), rng.standard_normal(ntaps)
                got = emul_mf(emul, tmp_path, x, b, start, step, xs, ys)
                assert np.array_equal(got, ss.matched_filter_rows_host(x, b, start, step)), (step, ntaps, k, dt)
                i += 1
    # the starts at and beyond the row's end: one output, then none
    for step, ntaps, n in ((1, 7, 40), (3, 2049, 9), (8, 8, 300), (64, 7, 70)):
        x, b = signal_of(rng, (3, n), np.complex64), rng.standard_normal(ntaps)
        for start in (0, 5, n - 1, n, n + 3):
            got = emul_mf(emul, tmp_path, x, b, start, step, n + 4, None)
            assert got.shape == (3, max(0, -(-(n - start) // step))) and np.array_equal(got, ss.matched_filter_rows_host(x, b, start, step)), (step, ntaps, n, start)
    # the naive layout (the timing A/B) computes the same bits; the contracted form does not promise them
    x, b = signal_of(rng, (2, 1200), np.complex128), rng.standard_normal(97)
    want = ss.matched_filter_rows_host(x, b, 96, 8)
    assert np.array_equal(emul_mf(emul, tmp_path, x, b, 96, 8, naive=1), want)
    fused = emul_mf(emul, tmp_path, x, b, 96, 8, fma=1)
    assert np.max(np.abs(fused - want)) <= (2 * 97 + 2) * U * np.sum(np.abs(b)) * np.max(np.abs(x))
    assert i >= 60


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process): both kernels over more than one tile and row,
    on inputs inside exact-size allocations"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "pulse_emul_san", san)
    rng = np.random.default_rng(2605)
    for ns, ntaps, dt in ((1, 2049, np.float32), (3, 7, np.complex64), (8, 97, np.complex128), (64, 2049, np.float64), (64, 1, np.complex64)):
        T = shape_plan(exe, dt, ntaps, ns, 1)["T"]
        for n in (1, T + 1, 2 * T + 3):
            x, b = signal_of(rng, (3, n), dt), rng.standard_normal(ntaps)
            assert np.array_equal(emul_shape(exe, tmp_path, x, b, ns, 1 / 7.0, n + 2, n * ns + 1), ss.pulse_shape_rows_host(x, b, ns, 1 / 7.0))
        To = mf_plan(exe, dt, ntaps, 1, 0, ns)["To"]
        for k, start in ((1, 0), (To + 1, 5), (2 * To + 3, 2)):
            n = start + (k - 1) * ns + 1
            x, b = signal_of(rng, (3, n), dt), rng.standard_normal(ntaps)
            assert np.array_equal(emul_mf(exe, tmp_path, x, b, start, ns, n + 3, k + 2), ss.matched_filter_rows_host(x, b, start, ns))
        x = signal_of(rng, (2, 50), dt)
        assert emul_mf(exe, tmp_path, x, rng.standard_normal(ntaps), 53, ns).shape == (2, 0)
