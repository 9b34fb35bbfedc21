"""Carrier phase tracking over frame sets without a GPU: the NumPy host forms against results captured from the real reference
(tests/golden/gen_golden_carrier.py -> g27_carrier.npz, g27_conventions.json), the arithmetic recipe's own functions (sincos, the wrap, atan2) against
np.longdouble and NumPy, and the kernels walked thread by thread on the CPU (tests/host/carrier_emul.cpp) with every global and LDS access
bounds-checked, once more under -fsanitize=address,undefined as a stand-alone program.  DESIGN.md 4.22.

The bound against the reference.  Every case of the fixture carries S, the spread between the reference's float64 run and the same statements in
np.longdouble: the reference's own rounding noise as the loop amplifies it.  The host form stays within 16 S: this project's sincos and atan2 are held
to 2 ulp where libm's errors are below 1, and the rotation, the detector, the loop filter and the wrap add as many roundings again -- an order of
magnitude, rounded up to a power of two.  MQAM cases add 3e-15 max|z_prime|, the documented accuracy of the row scale against np.std.  a_hat is equal.
Between the host form, the emulation and the device the comparison is array_equal.

Measured (this file prints it): the worst ratio of an error to its bound is 0.099 (16-QAM, type 0); sincos_rad errs by at most 1.26 ulp."""
import json
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, synchronization as sync
from conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "g27_carrier.npz"))
CONV = json.load(open(os.path.join(ROOT, "tests", "golden", "g27_conventions.json")))
CASES, STEPS = json.loads(str(G["cases"])), json.loads(str(G["steps"]))
TWO_PI = 2 * np.pi
CODES = {np.dtype(np.complex64): 1, np.dtype(np.complex128): 3}
NAMES = _ffi.CAR_OUTPUTS


def circ(d):
    d = np.mod(np.abs(d), TWO_PI)
    return np.minimum(d, TWO_PI - d)


def noisy_rows(rng, nrow, n, mod_type, M, dt=np.complex128, sigma=0.05):
    """constellation points plus noise under a slow rotation: what a loop meets (locked or not, host and device must agree)"""
    if mod_type == "MQAM":
        x_m = 1 if M == 2 else int(round(np.sqrt(M))) - 1
        s = (2 * rng.integers(0, x_m + 1, (nrow, n)) - x_m) + 1j * (2 * rng.integers(0, x_m + 1, (nrow, n)) - x_m)
    elif M == 4:
        s = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (nrow, n))))
    else:
        s = np.exp(1j * 2 * np.pi * rng.integers(0, M, (nrow, n)) / M)
    w = sigma * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))
    phase = 0.2 + 2 * np.pi * 1e-3 * np.arange(n)[None, :] + 0.1 * np.arange(nrow)[:, None]
    return ((s + w) * np.exp(1j * phase)).astype(dt)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_covers_what_the_issue_lists():
    have = {(c["mod_type"], c["M"], c["type"], c["snr_db"], c["f0"], c["phi0"], c["BnTs"]) for c in CASES if not c["open_loop"] and c["phase_step"] is None}
    want = {("MPSK", 2, 0, 15, 1e-3, 0.3, 0.05), ("MPSK", 2, 1, 15, 1e-3, 0.3, 0.05), ("MPSK", 4, 0, 15, 1e-3, 0.3, 0.05), ("MPSK", 4, 1, 15, 1e-3, 0.3, 0.05),
            ("MPSK", 8, 0, 25, 1e-3, 0.2, 0.05), ("MPSK", 8, 1, 25, 5e-4, 0.2, 0.02), ("MPSK", 16, 0, 30, 0.0, 0.1, 0.02), ("MQAM", 4, 0, 20, 1e-3, 0.3, 0.05),
            ("MQAM", 16, 0, 30, 1e-3, 0.3, 0.05), ("MQAM", 16, 2, 30, 1e-3, 0.3, 0.05), ("MQAM", 16, 1, 30, 5e-4, 0.2, 0.05), ("MQAM", 64, 0, 40, 0.0, 0.1, 0.001),
            ("MQAM", 64, 2, 40, 2e-4, 0.1, 0.02), ("MQAM", 256, 1, 50, 1e-4, 0.05, 0.02), ("MQAM", 256, 2, 50, 1e-4, 0.05, 0.02)}
    assert have == want
    assert sum(c["open_loop"] for c in CASES) == 1 and [c["phase_step"] for c in CASES if c["phase_step"]] == [[0.4, 200]]
    for c in CASES:
        assert c["zeta"] == 0.707 and G[c["key"] + "_z"].shape == (600,) and G[c["key"] + "_z"].dtype == np.complex128
        assert 0 < c["S"] <= 1e-12 and c["min_margin"] >= 1e-6
    assert {(s["fn"], s["ns"]) for s in STEPS} == {(f, ns) for f in ("phase_step", "time_step") for ns in (1, 4)}
    for ns in (1, 4):
        assert {s["n_step"] for s in STEPS if s["ns"] == ns} >= {5, 96 // ns, 200}
    assert CONV["mpsk_above_4"]["script_set_np_int_to_int"] and "AttributeError" in CONV["mpsk_above_4"]["reference_raises"]


def test_numpy_still_behaves_as_the_fixture_records():
    obs = CONV["mod_of_a_negative_sum"]
    assert np.mod(obs["sum"], TWO_PI) == obs["np_mod"] == obs["fmod_plus_2pi"] == np.fmod(obs["sum"], TWO_PI) + TWO_PI
    assert obs["tiny_negative_gives_2pi"] and np.mod(-1e-20, TWO_PI) == TWO_PI and obs["zero_remainder"] == 0.0 == np.mod(-TWO_PI, TWO_PI)
    assert CONV["sign_of_zero"] == [0.0, 0.0] == [float(np.sign(0.0)), float(np.sign(-0.0))]
    assert all(np.rint(float(k)) == v for k, v in CONV["rint_ties"].items()) and np.rint(2.5) == 2.0 and np.rint(1.5) == 2.0
    with np.errstate(all="ignore"):
        q = np.complex128(complex(*CONV["quotient_by_zero_decision"]["z"])) / np.complex128(0j)
    assert repr(float(q.imag)) == CONV["quotient_by_zero_decision"]["imag"] == "-inf"
    assert CONV["quotient_by_sqrt2"]["is_product_with_reciprocal"] and (np.complex128(1 + 1j) / np.sqrt(2)).real == 1.0 / np.sqrt(2) != np.sqrt(0.5)
    assert float(1.0 / np.sqrt(2)).hex() == CONV["quotient_by_sqrt2"]["reciprocal"]


# ---------------------------------------------------------------------------------------------------------------- the host form against the reference
def test_host_form_stays_within_16_S_of_the_reference(capsys):
    worst, at = 0.0, None
    for c in CASES:
        k = c["key"]
        zp, ah, e, th = sync.DD_carrier_sync_host(G[k + "_z"], c["M"], c["BnTs"], c["zeta"], c["mod_type"], c["type"], c["open_loop"])
        assert np.array_equal(ah, G[k + "_a_hat"]), k
        bound = 16 * c["S"] + (3e-15 * np.max(np.abs(G[k + "_z_prime"])) if c["mod_type"] == "MQAM" else 0.0)
        errs = (np.max(np.abs(zp - G[k + "_z_prime"])), np.max(np.abs(e - G[k + "_e_phi"])), np.max(circ(th - G[k + "_theta_h"])))
        with capsys.disabled():
            print("%s %s M=%d type=%d: z_prime %.2e e_phi %.2e theta_h %.2e bound %.2e" % ((k, c["mod_type"], c["M"], c["type"]) + errs + (bound,)))
        if max(errs) / bound > worst:
            worst, at = max(errs) / bound, k
        assert max(errs) <= bound, (k, errs, bound)
    with capsys.disabled():
        print("worst ratio to the bound: %.3f (%s)" % (worst, at))


def test_rows_host_form_is_the_one_row_form_per_row_and_takes_a_gain_per_row():
    rng = np.random.default_rng(2701)
    x = noisy_rows(rng, 3, 70, "MQAM", 16)
    bn = np.array([0.01, 0.05, 0.1])
    rows = sync.DD_carrier_sync_rows_host(x, 16, bn, mod_type="MQAM", type=2)
    for r in range(3):
        one = sync.DD_carrier_sync_host(x[r], 16, float(bn[r]), mod_type="MQAM", type=2)
        assert all(np.array_equal(a[r], b) for a, b in zip(rows, one))
    wide = np.zeros((3, 5 + 4 * 70), dtype=x.dtype)
    wide[:, 5::4] = x
    assert all(np.array_equal(a, b) for a, b in zip(sync.DD_carrier_sync_rows_host(wide, 16, bn, mod_type="MQAM", type=2, start=5, step=4), rows))
    only = sync.DD_carrier_sync_rows_host(x, 16, bn, mod_type="MQAM", type=2, outputs=("theta_h", "z_prime"))
    assert len(only) == 2 and np.array_equal(only[0], rows[3]) and np.array_equal(only[1], rows[0])


def test_departures_raise_what_the_docstring_says():
    z = np.ones(8, dtype=np.complex128)
    for bad in (dict(M=3), dict(M=64), dict(M=8, mod_type="MQAM"), dict(M=4, mod_type="PAM"), dict(M=4, type=3)):
        kw = dict(dict(M=4, mod_type="MPSK", type=0), **bad)
        with pytest.raises(ValueError):
            sync.DD_carrier_sync_host(z, kw["M"], 0.05, mod_type=kw["mod_type"], type=kw["type"])
    with pytest.raises(TypeError):
        sync.DD_carrier_sync_host(np.ones(8), 4, 0.05)
    with pytest.raises(ValueError):
        sync.DD_carrier_sync_rows_host(np.ones((2, 8), dtype=np.complex128), 4, np.array([0.1, 0.2, 0.3]))
    with pytest.raises(ValueError):
        sync.DD_carrier_sync_rows_host(np.ones((2, 8), dtype=np.complex128), 4, 0.1, outputs=("z_prime", "phase"))
    with pytest.raises(ValueError):
        sync.time_step_rows_host(np.ones((2, 8), dtype=np.complex128), 1, np.array([1, 7]), 5)      # rows of different lengths
    # a zero decision: np.sign(0) = 0; type 2 divides by it as NumPy does
    with np.errstate(all="ignore"):
        zp, ah, e, th = sync.DD_carrier_sync_host(np.array([0j, 1 + 1j]), 4, 0.05, type=2)
    assert ah[0] == 0 and np.isnan(e[0]) and np.isnan(th[1])
    zp, ah, e, th = sync.DD_carrier_sync_host(np.array([1j, 1 + 1j]), 2, 0.05, type=0)
    assert ah[0] == 0 and e[0] == 0 and th[0] == 0
    # complex64 is storage only
    x = noisy_rows(np.random.default_rng(5), 1, 50, "MPSK", 4, np.complex64)[0]
    got, wide = sync.DD_carrier_sync_host(x, 4, 0.05), sync.DD_carrier_sync_host(x.astype(np.complex128), 4, 0.05)
    assert got[0].dtype == got[1].dtype == np.complex64 and got[2].dtype == got[3].dtype == np.float64
    assert np.array_equal(got[0], wide[0].astype(np.complex64)) and np.array_equal(got[2], wide[2]) and np.array_equal(got[3], wide[3])


def test_phase_step_and_time_step_equal_the_reference():
    for s in STEPS:
        z, want = G[s["key"] + "_z"], G[s["key"] + "_y"]
        one, rows = (sync.phase_step_host, sync.phase_step_rows_host) if s["fn"] == "phase_step" else (sync.time_step_host, sync.time_step_rows_host)
        got = one(z, s["ns"], s["step"], s["n_step"])
        assert got.dtype == want.dtype and np.array_equal(got, want), s
        z2 = np.stack([z, z[::-1], 2 * z])
        per = np.full(3, s["step"])
        for step in (s["step"], per):
            got2 = rows(z2, s["ns"], step, s["n_step"])
            assert np.array_equal(got2[0], want) and np.array_equal(got2[2], one(2 * z, s["ns"], s["step"], s["n_step"])), s
    z2 = np.stack([G["p00_z"], G["p00_z"]])
    got = sync.phase_step_rows_host(z2, 1, np.array([0.4, -1.1]), 5)
    f = complex(np.exp(1j * np.array([-1.1]))[0])           # (scalar products: NumPy's ARRAY product fuses on some CPUs, g27_conventions.json)
    assert np.array_equal(got[0], G["p00_y"]) and np.array_equal(got[1, 5:], np.array([complex(v) * f for v in z2[1, 5:]]))
    got = sync.time_step_rows_host(z2, 4, np.array([3, 1]), 5)
    assert np.array_equal(got[1], np.hstack((z2[1, :20], z2[1, 21:], np.zeros(1))))


# ---------------------------------------------------------------------------------------------------------------- the recipe's own functions
def angles():
    rng = np.random.default_rng(2702)
    q = np.arange(9) * np.pi / 4
    return np.concatenate([rng.uniform(0.0, TWO_PI, 100000), q, np.nextafter(q, 10.0), np.nextafter(q, -10.0)[1:], [TWO_PI, np.nextafter(TWO_PI, 0.0)]])


def test_sincos_rad_is_within_2_ulp_of_longdouble(capsys):
    x = angles()
    s, c = _ffi.sincos_rad_host(x)
    xl = x.astype(np.longdouble)
    worst = 0.0
    for got, true in ((s, np.sin(xl)), (c, np.cos(xl))):
        ulp = np.spacing(np.abs(true.astype(np.float64)))
        worst = max(worst, float(np.max(np.abs(got.astype(np.longdouble) - true) / ulp)))
    with capsys.disabled():
        print("sincos_rad: worst error %.3f ulp over %d angles" % (worst, x.size))
    assert worst <= 2.0
    sm, cm = _ffi.sincos_rad_host(-x)                       # odd and even, to the bit (the type-1 detector's argument has either sign)
    assert np.array_equal(sm, -s) and np.array_equal(cm, c)
    assert np.all(np.isnan(_ffi.sincos_rad_host(np.array([np.nan, np.inf, 9.0]))))


def test_the_wrap_is_numpy_mod_exactly():
    a = np.concatenate([np.linspace(-50.0, 50.0, 200001), np.random.default_rng(2703).uniform(-50, 50, 100000), np.nextafter(0.0, [1.0, -1.0]),
                        np.nextafter(TWO_PI, [0.0, 10.0]), np.nextafter(-TWO_PI, [0.0, -10.0]), [0.0, -0.0, TWO_PI, -TWO_PI, -1e-20, 1e-20, 1e300, -1e300]])
    assert np.array_equal(_ffi.wrap_2pi_host(a), np.mod(a, TWO_PI))
    assert not np.any(np.signbit(_ffi.wrap_2pi_host(np.array([-TWO_PI, -0.0]))))


def test_atan2_restatement_is_rounded_to_nearest():
    rng = np.random.default_rng(2704)
    y, x = rng.standard_normal(100000), rng.standard_normal(100000)
    got, true = _ffi.atan2_rn_host(y, x), np.arctan2(y.astype(np.longdouble), x.astype(np.longdouble))
    assert np.max(np.abs(got.astype(np.longdouble) - true) / np.spacing(np.abs(got))) <= 0.5 + 2 ** -9      # (the yardstick itself carries 2^-11 ulp)
    assert np.array_equal(_ffi.atan2_rn_host(np.array([0.0, -0.0, 0.0, 1.0, -1.0]), np.array([1.0, -1.0, -1.0, 0.0, 0.0])),
                          np.arctan2(np.array([0.0, -0.0, 0.0, 1.0, -1.0]), np.array([1.0, -1.0, -1.0, 0.0, 0.0])))


def test_the_built_library_exports_the_new_symbols():
    L = _ffi.load()
    names = ["skdsp_carrier_rows", "skdsp_carrier_rows_dev", "skdsp_phase_step_rows_dev", "skdsp_time_step_rows_dev"]
    assert all(n in _ffi.SYMBOLS and hasattr(L, n) for n in names)
    header = open(os.path.join(ROOT, "include", "skdsp.h")).read()
    assert all(("int %s(" % n) in header for n in names)


# ---------------------------------------------------------------------------------------------------------------- the emulation
def build_emul(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "carrier_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("carrier"), "carrier_emul", [])


def words(exe, *args):
    return [int(w) for w in subprocess.check_output([exe] + [str(a) for a in args]).decode().split()]


def gaps_checked(raw, dt, nrow, n, stride):
    """the rows of an output block; the bytes between the rows must still hold the fill"""
    esz = np.dtype(dt).itemsize
    assert len(raw) == (((nrow - 1) * stride + n) * esz if nrow and n else 0)
    buf = np.frombuffer(raw, dtype=np.uint8)
    for r in range(nrow - 1):
        assert np.all(buf[(r * stride + n) * esz:(r + 1) * stride * esz] == 0xA5), "a gap between two output rows was written"
    flat = np.frombuffer(raw, dtype=dt)
    return np.stack([flat[r * stride:r * stride + n] for r in range(nrow)]) if nrow and n else np.zeros((nrow, n), dtype=dt)


def emul_rows(exe, tmp, x, mod_type, M, BnTs, type=0, open_loop=False, start=0, step=1, outputs=NAMES, r=None, y_stride=None):
    """x: (nrow, width), read as x[:, start::step]; the file holds what the call may read and not an element more"""
    fam = _ffi.carrier_family(mod_type)
    nrow, width = x.shape
    n = _ffi.sym_count(width, start, step)
    ys = n if y_stride is None else y_stride
    span = start + (n - 1) * step + 1 if n else 0
    k1, k2, gains = _ffi.carrier_gains_rows(BnTs, 0.707, nrow)
    inv, tre, tim = _ffi.carrier_table(fam, M)
    f = {k: os.path.join(str(tmp), k + ".bin") for k in ("gains", "r", "tab", "x")}
    (np.zeros(0) if gains is None else gains).tofile(f["gains"])
    (np.zeros(0) if r is None else np.asarray(r, dtype=np.float64)).tofile(f["r"])
    (np.zeros(0) if tre is None else np.stack([tre, tim], axis=1)).tofile(f["tab"])
    x.reshape(-1)[:(nrow - 1) * width + span if nrow and n else 0].tofile(f["x"])
    mask = sum(1 << NAMES.index(o) for o in outputs)
    prefix = os.path.join(str(tmp), "out_")
    subprocess.check_call([exe, "rows", str(CODES[x.dtype]), str(fam), str(M), str(type), str(int(open_loop)), str(mask), str(n), str(nrow), str(start), str(step), str(width),
                           str(ys), float(k1).hex(), float(k2).hex(), "0" if gains is None else "1", inv.hex(), f["gains"], f["r"], f["tab"], f["x"], prefix])
    dts = dict(z_prime=x.dtype, a_hat=x.dtype, e_phi=np.float64, theta_h=np.float64)
    return tuple(gaps_checked(open(prefix + o[0] + ".bin", "rb").read(), dts[o], nrow, n, ys) for o in outputs)


PAIRS = [("MPSK", 4, 0), ("MPSK", 2, 1), ("MPSK", 8, 0), ("MPSK", 16, 1), ("MPSK", 4, 2), ("MQAM", 16, 0), ("MQAM", 4, 1), ("MQAM", 64, 2), ("MQAM", 256, 2), ("MQAM", 2, 0)]


def test_plan_is_what_the_design_says(emul):
    lanes, T, pitch = words(emul, "plan")
    assert (lanes, T, pitch) == (64, 8, 9) and pitch % 2 == 1
    assert words(emul, "lds", 1) == [2 * 64 * pitch] and words(emul, "lds", 15) == [6 * 64 * pitch] and words(emul, "lds", 9) == [3 * 64 * pitch]
    assert 6 * 64 * pitch * 8 <= 64 * 1024


def test_emulated_functions_equal_their_numpy_restatements(emul, tmp_path):
    rng = np.random.default_rng(2705)
    a = np.concatenate([angles(), -angles()[:2000], rng.uniform(-50, 50, 5000), [0.0, -0.0, 1e-300]])
    b = rng.standard_normal(a.size)
    b[:100] = 0.0
    np.stack([a, b], axis=1).tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([emul, "funcs", str(a.size), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 6)
    s, c = _ffi.sincos_rad_host(a)
    assert np.array_equal(out[:, 0], s, equal_nan=True) and np.array_equal(out[:, 1], c, equal_nan=True)
    assert np.array_equal(out[:, 2], _ffi.wrap_2pi_host(a)) and np.array_equal(out[:, 2], np.mod(a, TWO_PI))
    assert np.array_equal(out[:, 3], _ffi.atan2_rn_host(a, b))
    assert np.array_equal(out[:, 4], np.sign(a))
    with np.errstate(all="ignore"):
        pick = np.arange(0, a.size, 5)                # NumPy's own complex division, on scalars (array loops are dispatched by CPU)
        want = np.array([(np.complex128(complex(a[i], b[i])) / np.complex128(complex(b[i], a[i]))).imag for i in pick])
        assert np.array_equal(out[pick, 5], want, equal_nan=True)


def test_emulated_kernel_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(2706)
    T = words(emul, "plan")[1]
    sizes = (0, 1, T - 1, T, T + 1, 3 * T + 5)
    i = 0
    for mod_type, M, det in PAIRS:
        for dt in (np.complex128, np.complex64):
            nrow, n = (1, 63, 64, 65, 130)[i % 5], sizes[(i // 2) % 6]
            start, step = ((0, 1), (5, 4), (3, 7))[i % 3]
            width = start + max(n - 1, 0) * step + (1 if n else 0) + (i % 2 if step > 1 and n else 0)
            sym = noisy_rows(rng, nrow, n, mod_type, M, dt)
            x = (100 * (rng.standard_normal((nrow, width)) + 1j)).astype(dt)                # what lies between the symbols must not matter
            x[:, start::step][:, :n] = sym
            assert _ffi.sym_count(width, start, step) == n
            bn = 0.05 if i % 4 else rng.uniform(0.01, 0.1, nrow)
            r = _ffi.qam_scale_rows_np(x, M, start, step) if mod_type == "MQAM" else None
            want = sync.DD_carrier_sync_rows_host(x, M, bn, mod_type=mod_type, type=det, open_loop=i % 7 == 3, start=start, step=step, r=r)
            got = emul_rows(emul, tmp_path, x, mod_type, M, bn, det, i % 7 == 3, start, step, r=r, y_stride=n + (i % 3))
            for name, g, w in zip(NAMES, got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), (mod_type, M, det, dt, nrow, n, name)
            i += 1
    # an unlocked high-order loop: type 0 on 256-QAM at an ordinary bandwidth drives |e_phi| into the tens, and the wrap stays exact
    x = noisy_rows(rng, 2, 3 * T + 5, "MQAM", 256)
    r = _ffi.qam_scale_rows_np(x, 256)
    want = sync.DD_carrier_sync_rows_host(x, 256, 0.05, mod_type="MQAM", type=0, r=r)
    assert np.max(np.abs(want[2])) > 10 and all(np.array_equal(g, w) for g, w in zip(emul_rows(emul, tmp_path, x, "MQAM", 256, 0.05, 0, r=r), want))
    # every subset of the outputs: the same arrays, nothing else written
    x = noisy_rows(rng, 65, 2 * T + 3, "MPSK", 8)
    full = sync.DD_carrier_sync_rows_host(x, 8, 0.05, type=1)
    for mask in range(1, 16):
        outs = tuple(o for j, o in enumerate(NAMES) if mask >> j & 1)
        got = emul_rows(emul, tmp_path, x, "MPSK", 8, 0.05, 1, outputs=outs, y_stride=2 * T + 4)
        assert all(np.array_equal(g, full[NAMES.index(o)]) for g, o in zip(got, outs)), outs


def emul_imp(exe, tmp, z, mode, ns, n_step, step, n_out, x_stride=None, y_stride=None):
    nrow, n = z.shape
    xs, ys = n if x_stride is None else x_stride, n_out if y_stride is None else y_stride
    per = np.ndim(step) > 0
    flat = np.zeros((nrow - 1) * xs + n, dtype=z.dtype)
    for r in range(nrow):
        flat[r * xs:r * xs + n] = z[r]
    f = {k: os.path.join(str(tmp), k + ".bin") for k in ("vals", "x", "y")}
    flat.tofile(f["x"])
    c, d, shift = 1.0, 0.0, 0
    vals = np.zeros(0)
    if mode == 1:
        fac = np.exp(1j * np.atleast_1d(np.asarray(step, dtype=np.float64)))
        vals, c, d = (np.stack([fac.real, fac.imag], axis=1), c, d) if per else (vals, float(fac[0].real), float(fac[0].imag))
    else:
        vals, shift = (np.asarray(step, dtype=np.int64), 0) if per else (vals, int(step))
    vals.tofile(f["vals"])
    subprocess.check_call([exe, "imp", str(mode), str(CODES[z.dtype]), str(n), str(n_out), str(nrow), str(ns), str(n_step), str(xs), str(ys), str(shift), str(int(per)),
                           float(c).hex(), float(d).hex(), f["vals"], f["x"], f["y"]])
    return gaps_checked(open(f["y"], "rb").read(), z.dtype, nrow, n_out, ys)


def test_emulated_impairment_kernel_equals_the_host_forms_and_the_reference(emul, tmp_path):
    for s in STEPS:
        z, want = G[s["key"] + "_z"], G[s["key"] + "_y"]
        mode = 1 if s["fn"] == "phase_step" else 0
        got = emul_imp(emul, tmp_path, z.reshape(1, -1), mode, s["ns"], s["n_step"], s["step"], want.size)
        assert np.array_equal(got[0], want), s
    rng = np.random.default_rng(2707)
    for dt in (np.complex64, np.complex128):
        z = (rng.standard_normal((5, 301)) + 1j * rng.standard_normal((5, 301))).astype(dt)
        for ns in (1, 4):
            for n_step in (0, 7, -(-301 // ns), 400):
                p = rng.uniform(-3, 3, 5)
                want = sync.phase_step_rows_host(z, ns, p, n_step)
                assert np.array_equal(emul_imp(emul, tmp_path, z, 1, ns, n_step, p, want.shape[1], 310, want.shape[1] + 3), want)
                want = sync.time_step_rows_host(z, ns, 3, n_step)
                assert np.array_equal(emul_imp(emul, tmp_path, z, 0, ns, n_step, 3, want.shape[1], 301, want.shape[1] + 1), want)
        want = sync.time_step_rows_host(z, 4, np.array([0, 1, 2, 3, 9]), 20)
        assert np.array_equal(emul_imp(emul, tmp_path, z, 0, 4, 20, np.array([0, 1, 2, 3, 9]), 301), want)


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process): the loop kernel over more than one tile and
    group for every (family, type) pair, the impairment kernel, on inputs inside exact-size allocations"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "carrier_emul_san", san)
    rng = np.random.default_rng(2708)
    for i, (mod_type, M, det) in enumerate(PAIRS):
        dt = (np.complex64, np.complex128)[i % 2]
        start, step = ((0, 1), (5, 4), (3, 7))[i % 3]
        n = 2 * 8 + 3
        x = np.zeros((65, start + (n - 1) * step + 1), dtype=dt)
        x[:, start::step] = noisy_rows(rng, 65, n, mod_type, M, dt)
        r = _ffi.qam_scale_rows_np(x, M, start, step) if mod_type == "MQAM" else None
        want = sync.DD_carrier_sync_rows_host(x, M, 0.05, mod_type=mod_type, type=det, start=start, step=step, r=r)
        got = emul_rows(exe, tmp_path, x, mod_type, M, 0.05, det, False, start, step, r=r, y_stride=n + 1)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)), (mod_type, M, det)
    z = (rng.standard_normal((3, 97)) + 1j * rng.standard_normal((3, 97))).astype(np.complex64)
    assert np.array_equal(emul_imp(exe, tmp_path, z, 1, 4, 7, 0.4, 25), sync.phase_step_rows_host(z, 4, 0.4, 7))
    assert np.array_equal(emul_imp(exe, tmp_path, z, 0, 4, 7, 3, 97), sync.time_step_rows_host(z, 4, 3, 7))
    assert np.array_equal(emul_imp(exe, tmp_path, z, 0, 4, 30, 3, 100), sync.time_step_rows_host(z, 4, 3, 30))
