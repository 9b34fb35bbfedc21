"""Symbol timing recovery over frame sets without a GPU: the NumPy host form against results captured from the real reference
(tests/golden/gen_golden_nda.py -> g28_nda.npz, g28_conventions.json), and the kernels walked thread by thread on the CPU (tests/host/nda_emul.cpp) with
every global and LDS access bounds-checked, once more under -fsanitize=address,undefined as a stand-alone program.  DESIGN.md 4.23.

The bound against the reference.  Every case of the fixture carries S, the spread between the reference's float64 run and the same statements in
np.longdouble: the reference's own rounding noise as the loop amplifies it.  The host form's raw zz and e_tau stay within 16 S, the project's bound for a
loop of this kind (test_carrier_cpu.py): the project's atan2 and |z|^2 differ from libm's by an ulp or two, as many roundings again elsewhere, rounded
up to a power of two.  Normalised zz stays within (16 S + A max|zz_raw|) / std with A = 3e-15, the accuracy of the rows' standard deviation against
np.std (two passes with tree sums: (n / 512 + 8) 2^-53 relative, below 3e-15 up to 8192 symbols).  counts and the underflow samples are equal.
Between the host form, the emulation and the device the comparison is array_equal.

Measured (this file prints it): the worst ratio of an error to its bound is 0.155 (raw, Ns = 3, I_ord = 2) and 0.036 (normalised); the rows' standard
deviation is within 1.7e-16 (relative) of np.std evaluated in np.longdouble."""
import json
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, synchronization as sync
from conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "g28_nda.npz"))
CONV = json.load(open(os.path.join(ROOT, "tests", "golden", "g28_conventions.json")))
CASES = json.loads(str(G["cases"]))
CODES = {np.dtype(np.complex64): 1, np.dtype(np.complex128): 3}
NAMES = _ffi.NDA_OUTPUTS
A_STD = 3e-15


def case_input(c):
    z = G[c["signal"]]
    return z[:z.size - c["trim"]]


def frames(rng, nrow, n, Ns, dt=np.complex128, sigma=0.05):
    """QPSK through a triangular pulse of two symbols, a different timing phase per row, plus noise: what a loop meets"""
    nsym = n // Ns + 3
    s = (2 * rng.integers(0, 2, (nrow, nsym)) - 1) + 1j * (2 * rng.integers(0, 2, (nrow, nsym)) - 1)
    t = (np.arange(n)[None, :] + rng.uniform(0, Ns, (nrow, 1))) / Ns
    k = t.astype(int)
    x = np.take_along_axis(s, k, 1) * (1 - (t - k)) + np.take_along_axis(s, k + 1, 1) * (t - k)
    return (x + sigma * (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n)))).astype(dt)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_covers_what_the_issue_lists():
    plain = [c for c in CASES if c["signal"] in ("s3", "s4", "s8")]
    assert {(c["Ns"], c["I_ord"]) for c in plain if c["L"] == 2 and c["BnTs"] == 0.01 and c["trim"] == 0} == {(ns, i) for ns in (3, 4, 8) for i in (1, 2, 3)}
    assert {c["L"] for c in plain if c["Ns"] == 4} == {0, 1, 2, 4} and {c["BnTs"] for c in plain if c["Ns"] == 4} == {0.005, 0.01, 0.02, 0.05}
    assert {case_input(c).size % 4 for c in plain if c["Ns"] == 4} == {0, 1, 2, 3}
    assert sorted(c["signal"] for c in CASES if c["signal"] not in ("s3", "s4", "s8")) == ["n4", "q4", "t4"]
    assert all(c["Ns"] != 2 and c["zeta"] == 0.707 for c in CASES)
    for c in CASES:
        z = case_input(c)
        assert z.dtype == np.complex128 and z.size in range(c["Ns"] * 300 - 3, c["Ns"] * 300 + 1)
        assert 0 < c["S"] <= 1e-12 and c["margin"] >= 1e-9 and c["max_e"] <= 0.5 - 1e-6
        assert G[c["key"] + "_zz"].shape == G[c["key"] + "_e_tau"].shape == G[c["key"] + "_raw"].shape and G[c["key"] + "_zz"].size > 290
        assert c["std"] == float(np.std(G[c["key"] + "_raw"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g28_nda.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g27_carrier.npz"))


def sum_model(x):
    """g28_conventions.json's complex_sum_order, through the host form's own np_csum_host"""
    sr, si = _ffi.np_csum_host([(np.float64(v.real), np.float64(v.imag)) for v in x])
    return complex(sr, si)


def test_numpy_still_behaves_as_the_fixture_records():
    rng = np.random.default_rng(2801)
    assert all(CONV["complex_sum_order"]["holds_for_lengths"][str(n)] for n in range(1, 18))
    for n in range(1, 18):
        for _ in range(200):
            x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 10.0 ** rng.integers(-8, 8, n)
            assert complex(np.sum(x)) == sum_model(x), n
    for _ in range(200):                                   # the Farrow statement: a reversed slice times a list, summed
        z = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * 10.0 ** rng.integers(-8, 8, 6)
        co = [-1 / 6., 1, -1 / 2., -1 / 3.]
        want = complex(np.sum(z[4:0:-1] * co))
        a = (z[1], z[2], z[3], z[4])
        assert want == complex(_ffi._farrow_sum_host([v.real for v in a], co), _ffi._farrow_sum_host([v.imag for v in a], co))
    a = np.complex128(0.3 - 0.7j)
    assert CONV["complex_scalar_by_int_is_product_with_reciprocal"] and all((a / d).real == a.real * (1.0 / d) and (a / d).imag == a.imag * (1.0 / d) for d in (3, 5, 7, 17))
    arr = rng.standard_normal(9) + 1j * rng.standard_normal(9)
    s = np.std(arr)
    div = arr.copy()
    div /= s
    assert CONV["std"]["in_place_division_is_product_with_reciprocal"] and np.array_equal(div.real, arr.real * (1.0 / s)) and np.array_equal(div.imag, arr.imag * (1.0 / s))
    assert CONV["float_times_complex_scalar_is_per_component"] and (np.float64(0.3) * a).imag == 0.3 * a.imag
    for key, N in CONV["loop_range"]["N_of_len"].items():
        ns, n = (int(v) for v in key.split(","))
        assert _ffi.nda_loop_end(n, ns) == max(0, N), key
    assert CONV["first_underflow_at_nn"] == 1 and CONV["first_interpolant_at_nn"] == 2 and CONV["stores_start_at_index_1"]
    assert CONV["final_trim"]["outputs_equal_heavy_steps"] and CONV["std"]["no_outputs"] == {"len_z": 5, "zz_size": 0, "e_tau_size": 0}
    assert "nan" in CONV["std"]["one_output"]["zz"] and CONV["std"]["one_output"]["e_tau"] == [0.0]
    # only odd lengths ever made the reference's slices run past its array
    assert all(int(n) % 2 == 1 for per in CONV["ns2_slices_past_the_array"]["probe_len_to_error_by_I_ord"].values() for n, err in per.items() if err)


def test_reference_conventions_hold_in_the_host_form():
    z = G["s4"]
    zz, e = sync.NDA_symb_sync_host(z[:5], 4, 2, 0.01)
    assert zz.size == e.size == 0 and zz.dtype == np.complex128 and e.dtype == np.float64
    zz, e = sync.NDA_symb_sync_host(z[:15], 4, 2, 0.01)
    assert zz.size == 1 and np.isnan(zz[0].real) and np.isnan(zz[0].imag) and e.tolist() == [0.0]
    zz, e, counts, marks = _ffi.nda_rows_host(z.reshape(1, -1), 4, 2, 0.01, underflows=True)
    assert marks[0][0] == 1 and zz[0, 0] == 0 and e[0, 0] == 0 and e[0, 1] != 0 and counts[0] == sum(1 for u in marks[0] if u + 1 <= _ffi.nda_loop_end(z.size, 4) - 1)
    assert zz.shape == e.shape == (1, _ffi.nda_iters(z.size, 4)) and not np.any(zz[0, counts[0]:]) and not np.any(e[0, counts[0]:])
    # a non-finite sample ends its own row's symbols as in the reference, and touches no other row
    rows = np.stack([z, z, z])
    rows[1, 600] = np.nan
    zz3, e3, c3 = sync.NDA_symb_sync_rows_host(rows, 4, 2, 0.01)
    probe = CONV["non_finite_sample"]
    assert c3.tolist() == [probe["outputs_without"], probe["outputs_with"], probe["outputs_without"]] and np.all(np.isnan(zz3[1, :c3[1]])) == probe["all_zz_nan"]
    assert int(np.sum(np.isnan(e3[1]))) == probe["e_tau_nan_count"] and np.array_equal(zz3[0], zz[0]) and np.array_equal(zz3[2], zz[0]) and np.array_equal(e3[2], e[0])


# ---------------------------------------------------------------------------------------------------------------- the host form against the reference
def test_host_form_stays_within_16_S_of_the_reference(capsys):
    worst_raw, worst_norm, worst_std, at = 0.0, 0.0, 0.0, None
    for c in CASES:
        k, z = c["key"], case_input(c).reshape(1, -1)
        raw, e, counts, marks = _ffi.nda_rows_host(z, c["Ns"], c["L"], c["BnTs"], c["zeta"], c["I_ord"], normalize=False, underflows=True)
        n = int(counts[0])
        assert n == G[k + "_e_tau"].size and marks[0] == G[k + "_under"].tolist(), k
        bound = 16 * c["S"]
        errs = (float(np.max(np.abs(raw[0, :n] - G[k + "_raw"]))), float(np.max(np.abs(e[0, :n] - G[k + "_e_tau"]))))
        zz, e2 = sync.NDA_symb_sync_host(z[0], c["Ns"], c["L"], c["BnTs"], c["zeta"], c["I_ord"])
        bound_n = (16 * c["S"] + A_STD * np.max(np.abs(G[k + "_raw"]))) / c["std"]
        err_n = float(np.max(np.abs(zz - G[k + "_zz"])))
        std = float(_ffi.nda_std_rows_host(raw, counts)[0])
        true = np.std(G[k + "_raw"].astype(np.clongdouble))
        err_s = float(abs(np.longdouble(std) - true) / true)
        with capsys.disabled():
            print("%s Ns=%d L=%d BnTs=%g I_ord=%d: raw zz %.2e e_tau %.2e bound %.2e | zz %.2e bound %.2e | std rel %.2e" % ((k, c["Ns"], c["L"], c["BnTs"], c["I_ord"]) + errs +
                                                                                                                     (bound, err_n, bound_n, err_s)))
        if max(errs) / bound > worst_raw:
            worst_raw, at = max(errs) / bound, k
        worst_norm, worst_std = max(worst_norm, err_n / bound_n), max(worst_std, err_s)
        assert np.array_equal(e2, e[0, :n]) and max(errs) <= bound and err_n <= bound_n and err_s <= A_STD, (k, errs, bound, err_n, bound_n, err_s)
    with capsys.disabled():
        print("worst ratio to the bound: raw %.3f (%s), normalised %.3f; worst std error %.2e" % (worst_raw, at, worst_norm, worst_std))


def test_rows_host_form_is_the_one_row_form_per_row_and_takes_a_gain_per_row():
    rng = np.random.default_rng(2802)
    x = frames(rng, 3, 90, 4)
    bn = np.array([0.01, 0.05, 0.1])
    zz, e, counts = sync.NDA_symb_sync_rows_host(x, 4, 1, bn, I_ord=2)
    for r in range(3):
        one = sync.NDA_symb_sync_host(x[r], 4, 1, float(bn[r]), I_ord=2)
        assert np.array_equal(zz[r, :counts[r]], one[0]) and np.array_equal(e[r, :counts[r]], one[1]) and not np.any(zz[r, counts[r]:])
    wide = np.concatenate([100 * np.ones((3, 7)), x], axis=1)
    assert all(np.array_equal(a, b) for a, b in zip(sync.NDA_symb_sync_rows_host(wide, 4, 1, bn, I_ord=2, start=7), (zz, e, counts)))
    only = sync.NDA_symb_sync_rows_host(x, 4, 1, bn, I_ord=2, outputs=("e_tau",))
    assert len(only) == 2 and np.array_equal(only[0], e) and np.array_equal(only[1], counts)
    raw = sync.NDA_symb_sync_rows_host(x, 4, 1, bn, I_ord=2, normalize=False)[0]
    with np.errstate(all="ignore"):
        assert np.allclose(zz, raw / np.array([np.std(raw[r, :counts[r]]) for r in range(3)])[:, None], rtol=1e-14, atol=0)
    # complex64 is storage only; a real z is widened exactly
    x32 = x.astype(np.complex64)
    got, ref = sync.NDA_symb_sync_rows_host(x32, 4, 1, bn), sync.NDA_symb_sync_rows_host(x32.astype(np.complex128), 4, 1, bn)
    assert got[0].dtype == np.complex64 and got[1].dtype == np.float64 and np.array_equal(got[0], ref[0].astype(np.complex64)) and np.array_equal(got[1], ref[1])
    for dt, cdt in ((np.float32, np.complex64), (np.float64, np.complex128)):
        xr = x.real.astype(dt)
        a, b = sync.NDA_symb_sync_rows_host(xr, 4, 1, 0.02), sync.NDA_symb_sync_rows_host(xr.astype(cdt), 4, 1, 0.02)
        assert a[0].dtype == cdt and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def test_errors_raise_what_the_docstring_says():
    z = frames(np.random.default_rng(2803), 2, 60, 4)
    for bad in (dict(Ns=1), dict(Ns=17), dict(Ns=4.0), dict(L=-1), dict(L=9), dict(L=1.5), dict(I_ord=0), dict(I_ord=4), dict(I_ord=2.0)):
        kw = dict(dict(Ns=4, L=2, I_ord=3), **bad)
        with pytest.raises(ValueError):
            sync.NDA_symb_sync_host(z[0], kw["Ns"], kw["L"], 0.01, I_ord=kw["I_ord"])
        with pytest.raises(ValueError):
            sync.NDA_symb_sync_rows_host(z, kw["Ns"], kw["L"], 0.01, I_ord=kw["I_ord"])
    with pytest.raises(TypeError):
        sync.NDA_symb_sync_host(np.ones(60, dtype=np.int32), 4, 2, 0.01)
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_host(z, 4, 2, 0.01)                                    # one row, one dimension
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_rows_host(z[0], 4, 2, 0.01)
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_rows_host(z, 4, 2, np.array([0.1, 0.2, 0.3]))
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01, outputs=("zz", "phase"))
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01, start=61)
    with pytest.raises(ValueError):
        sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01, max_symbols=-1)
    # Ns = 2, I_ord >= 2: the lengths at which the reference's slices can run past its array
    for n in range(0, 12):
        for i_ord in (1, 2, 3):
            if n % 2 == 1 and n >= 3 and i_ord >= 2:
                with pytest.raises(ValueError):
                    sync.NDA_symb_sync_host(z[0, :n], 2, 1, 0.01, I_ord=i_ord)
            else:
                with np.errstate(all="ignore"):
                    sync.NDA_symb_sync_host(z[0, :n], 2, 1, 0.01, I_ord=i_ord)
    # more outputs than max_symbols: the rows are named
    counts = sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01)[2]
    with pytest.raises(ValueError, match=r"rows \[0, 1\]"):
        sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01, max_symbols=int(counts.min()) - 1)
    assert sync.NDA_symb_sync_rows_host(z, 4, 2, 0.01, max_symbols=int(counts.max()))[0].shape == (2, counts.max())


def test_the_built_library_exports_the_new_symbols():
    L = _ffi.load()
    names = ["skdsp_nda_rows", "skdsp_nda_rows_dev"]
    assert all(n in _ffi.SYMBOLS and hasattr(L, n) for n in names)
    header = open(os.path.join(ROOT, "include", "skdsp.h")).read()
    assert all(("int %s(" % n) in header for n in names)


# ---------------------------------------------------------------------------------------------------------------- the emulation
def build_emul(tmp, name, extra):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "nda_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("nda"), "nda_emul", [])


def words(exe, *args):
    return [int(w) for w in subprocess.check_output([exe] + [str(a) for a in args]).decode().split()]


def rows_checked(raw, dt, nrow, cap, stride, counts):
    """the rows of an output block, zero behind the counts; the bytes behind a row's count and between the rows must still hold the fill"""
    esz = np.dtype(dt).itemsize
    assert len(raw) == (((nrow - 1) * stride + cap) * esz if nrow and cap else 0)
    buf = np.frombuffer(raw, dtype=np.uint8)
    out = np.zeros((nrow, cap), dtype=dt)
    flat = np.frombuffer(raw, dtype=dt)
    for r in range(nrow if cap else 0):
        k = min(int(counts[r]), cap)
        end = (r + 1) * stride if r + 1 < nrow else r * stride + cap
        assert np.all(buf[(r * stride + k) * esz:end * esz] == 0xA5), "something behind a row's count was written"
        out[r, :k] = flat[r * stride:r * stride + k]
    return out


def emul_rows(exe, tmp, x, Ns, L, BnTs, I_ord=3, start=0, n=None, normalize=True, cap=None, outputs=NAMES, y_stride=None):
    """x: (nrow, width); a row's frame is x[r, start:start + n] (default: to the row's end); the file holds what the call may read and not an element more.
    Returns (zz, e_tau, counts) with None for an output that was not selected."""
    nrow, width = x.shape
    n = width - start if n is None else n
    cap = _ffi.nda_iters(n, Ns) if cap is None else cap
    ys = cap if y_stride is None else y_stride
    k1, k2, gains = _ffi.nda_gains_rows(BnTs, 0.707, Ns, nrow)
    rot, inv_ns, inv_len, k_eps = _ffi.nda_consts(Ns, L)
    f = {k: os.path.join(str(tmp), k + ".bin") for k in ("gains", "rot", "x")}
    (np.zeros(0) if gains is None else gains).tofile(f["gains"])
    rot.tofile(f["rot"])
    x.reshape(-1)[:(nrow - 1) * width + start + n if nrow and n else 0].tofile(f["x"])
    mask = sum(1 << NAMES.index(o) for o in outputs)
    prefix = os.path.join(str(tmp), "out_")
    subprocess.check_call([exe, "rows", str(CODES[x.dtype]), str(Ns), str(L), str(I_ord), str(mask), str(int(normalize)), str(n), str(nrow), str(start), str(width), str(ys),
                           str(cap), float(k1).hex(), float(k2).hex(), "0" if gains is None else "1", float(inv_ns).hex(), float(inv_len).hex(), float(k_eps).hex(),
                           f["gains"], f["rot"], f["x"], prefix])
    counts = np.fromfile(prefix + "c.bin", dtype=np.int64)
    assert counts.size == nrow
    zz = rows_checked(open(prefix + "z.bin", "rb").read(), x.dtype, nrow, cap, ys, counts) if "zz" in outputs else None
    e = rows_checked(open(prefix + "e.bin", "rb").read(), np.float64, nrow, cap, ys, counts) if "e_tau" in outputs else None
    return zz, e, counts


def test_plan_is_what_the_design_says(emul):
    for ns, L in ((2, 0), (4, 2), (16, 8)):
        lanes, T, W, pitch, lds, norm_threads = words(emul, "plan", ns, L)
        assert (lanes, T, W, norm_threads) == (64, 16, 16 + ns + 2, _ffi.NDA_NORM_THREADS) and pitch % 2 == 1 and pitch >= W
        assert lds == 2 * 64 * pitch + 2 * 64 * (2 * L + 1) and lds * 8 <= 64 * 1024
    for ns in (2, 3, 4, 8, 16):
        for n in (0, 1, ns * ns - ns - 1, ns * ns - ns, ns * ns, 100, 1201):
            assert words(emul, "iters", n, ns) == [_ffi.nda_iters(n, ns)]
            assert _ffi.nda_iters(n, ns) == max(0, len(range(1, ns * int(np.floor((n + 1) / float(ns) - (ns - 1))))))


def lengths_for(Ns, T):
    first = Ns * Ns - Ns
    return [0, 1, first - 1, first, T - 1, T, T + 1, 3 * T + 5] + [first + j for j in (T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)]


def test_emulated_kernel_equals_the_host_form(emul, tmp_path):
    rng = np.random.default_rng(2804)
    T = words(emul, "plan", 4, 0)[1]
    i = 0
    for Ns in (2, 3, 4, 8, 16):
        for n in lengths_for(Ns, T):
            I_ord, L, nrow = 1 + i % 3, (0, 2, 8)[(i // 3) % 3], (1, 63, 64, 65, 130)[i % 5]
            dt = (np.complex128, np.complex64)[(i // 2) % 2]
            if _ffi.nda_refused_length(n, Ns, I_ord):
                n += 1
            start, gap = (0, 5, 3)[i % 3], (0, 2)[i % 2]
            x = (100 * (rng.standard_normal((nrow, start + n + gap)) + 1j)).astype(dt)              # what lies around the frames must not matter
            x[:, start:start + n] = frames(rng, nrow, n, Ns, dt)
            bn = 0.02 if i % 4 else rng.uniform(0.005, 0.1, nrow)
            normalize = i % 3 != 1
            want = sync.NDA_symb_sync_rows_host(x[:, :start + n], Ns, L, bn, I_ord=I_ord, start=start, normalize=normalize)
            got = emul_rows(emul, tmp_path, x, Ns, L, bn, I_ord, start, n, normalize, y_stride=_ffi.nda_iters(n, Ns) + i % 3)
            for name, g, w in zip(NAMES + ("counts",), got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), (Ns, n, I_ord, L, nrow, dt, name)
            i += 1
    # rows driven out of lock: a loop bandwidth that takes W out of (0, 1) -- rows that underflow on every sample (W above 1) and rows that never do again (W below 0)
    x = frames(rng, 65, 3 * T + 30, 4)
    bn = rng.uniform(4.0, 12.0, 65)
    want = _ffi.nda_rows_host(x, 4, 2, bn, underflows=True)
    assert want[2].max() >= _ffi.nda_iters(x.shape[1], 4) - 4 and want[2].min() <= 2 and any(np.all(np.diff(m)[4:] == 1) for m in want[3] if len(m) > 8)
    got = emul_rows(emul, tmp_path, x, 4, 2, bn)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want[:3]))
    # max_symbols below a row's count: the kernel keeps counting, stores cap elements and nothing behind them
    x = frames(rng, 65, 4 * T + 3, 4, np.complex64)
    full = sync.NDA_symb_sync_rows_host(x, 4, 2, 0.02, normalize=False)
    cap = int(full[2].min()) - 2
    zz, e, counts = emul_rows(emul, tmp_path, x, 4, 2, 0.02, normalize=False, cap=cap, y_stride=cap + 1)
    assert np.array_equal(counts, full[2]) and np.array_equal(zz, full[0][:, :cap]) and np.array_equal(e, full[1][:, :cap])
    # every subset of the outputs: the same arrays
    x = frames(rng, 65, 2 * T + 19, 3)
    full = sync.NDA_symb_sync_rows_host(x, 3, 1, 0.02, I_ord=2)
    for outs in (("zz",), ("e_tau",), ("zz", "e_tau")):
        got = emul_rows(emul, tmp_path, x, 3, 1, 0.02, 2, outputs=outs)
        assert np.array_equal(got[2], full[2]) and all(np.array_equal(got[NAMES.index(o)], full[NAMES.index(o)]) for o in outs), outs
    # a NaN sample: its row alone
    x = frames(rng, 5, 3 * T, 4)
    clean = emul_rows(emul, tmp_path, x, 4, 2, 0.02)
    x[2, T + 3] = np.nan
    got, want = emul_rows(emul, tmp_path, x, 4, 2, 0.02), sync.NDA_symb_sync_rows_host(x, 4, 2, 0.02)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)) and got[2][2] < clean[2][2]
    assert all(np.array_equal(np.delete(g, 2, 0), np.delete(c, 2, 0)) for g, c in zip(got, clean))


def test_emulated_kernel_holds_the_golden_cases(emul, tmp_path):
    for c in CASES[::4]:
        z = case_input(c).reshape(1, -1)
        want = sync.NDA_symb_sync_rows_host(z, c["Ns"], c["L"], c["BnTs"], c["zeta"], c["I_ord"])
        got = emul_rows(emul, tmp_path, z, c["Ns"], c["L"], c["BnTs"], c["I_ord"])
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), c["key"]


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process): both kernels over more than one tile and group for
    every interpolator order, on inputs inside exact-size allocations"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "nda_emul_san", san)
    rng = np.random.default_rng(2805)
    for i, (Ns, I_ord, L) in enumerate([(2, 1, 0), (2, 3, 2), (3, 2, 1), (4, 3, 2), (8, 2, 8), (16, 3, 0), (4, 1, 4)]):
        dt = (np.complex64, np.complex128)[i % 2]
        n = Ns * Ns + 2 * 16 + 4 + i % 2
        if _ffi.nda_refused_length(n, Ns, I_ord):
            n += 1
        start = (0, 3)[i % 2]
        x = np.zeros((65, start + n), dtype=dt)
        x[:, start:] = frames(rng, 65, n, Ns, dt)
        want = sync.NDA_symb_sync_rows_host(x, Ns, L, 0.03, I_ord=I_ord, start=start)
        got = emul_rows(exe, tmp_path, x, Ns, L, 0.03, I_ord, start, y_stride=_ffi.nda_iters(n, Ns) + 1)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)), (Ns, I_ord, L)
    x = frames(rng, 3, 100, 4, np.complex64)
    full = sync.NDA_symb_sync_rows_host(x, 4, 2, 0.02, normalize=False)
    zz, e, counts = emul_rows(exe, tmp_path, x, 4, 2, 0.02, normalize=False, cap=5)
    assert np.array_equal(counts, full[2]) and np.array_equal(zz, full[0][:, :5])
