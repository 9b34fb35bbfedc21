"""Gray symbol mapping and demapping without a GPU: the NumPy yardsticks digitalcom.qam_gray_decode_host / mpsk_gray_decode_host and
_ffi.gray_map_rows_host against every result captured from the real reference (tests/golden/gen_golden_symmap.py -> g22_symmap.npz,
g22_conventions.json), the argument conventions of the public functions that need no device, and the kernels' plans, item geometry, staging,
decisions and merge of partial moments walked thread by thread on the CPU (tests/host/symmap_emul.cpp over csrc/symmap_core.hpp), once more
under -fsanitize=address,undefined as a stand-alone program.  Decisions and table lookups compare by array_equal; the scale against an exact
(math.fsum) evaluation of its definition, within the bounds of DESIGN.md 4.17."""
import inspect
import json
import math
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc
from conftest import GOLDEN, ROOT

QAM_ORDERS, MPSK_ORDERS = (2, 4, 16, 64, 256), (2, 4, 8, 16, 32)
FAMILIES = [(_ffi.QAM, m) for m in QAM_ORDERS] + [(_ffi.MPSK, m) for m in MPSK_ORDERS]
ROT = np.exp(-1j * np.pi / 4)


@pytest.fixture(scope="module")
def g22():
    g = np.load(os.path.join(GOLDEN, "g22_symmap.npz"))
    return g, {name: json.loads(str(g[name])) for name in ("dec", "spec", "map")}


@pytest.fixture(scope="module")
def conv22():
    return json.load(open(os.path.join(GOLDEN, "g22_conventions.json")))


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def test_fixture_covers_what_the_issue_lists(g22, conv22):
    g, lists = g22
    dec = lists["dec"]
    for fn, orders in (("qam_gray_decode", QAM_ORDERS), ("mpsk_gray_decode", MPSK_ORDERS)):
        for mod in orders:
            tags = {d["tag"] for d in dec if d["fn"] == fn and d["mod"] == mod}
            assert {"clean", "noisy", "c64w"} <= tags, (fn, mod, tags)
            assert fn != "qam_gray_decode" or {"offset", "c64"} <= tags
    assert any(d["tag"] == "real" and d["mod"] == 2 and d["in_dtype"] == "float64" for d in dec)
    for d in dec:       # every case within the size and above its margin bound, which is the issue's
        assert d["n"] <= 4096 and d["margin"] >= d["bound"] and d["bound"] == (2e-3 if d["tag"] == "c64" else 1e-6)
        assert d["out_dtype"] == ("int16" if d["fn"] == "qam_gray_decode" and d["mod"] == 2 else "int64")
    noisy = [d for d in dec if d["tag"] == "noisy"]
    assert all(not np.array_equal(g[d["key"] + "_out"], g[d["key"].replace("noisy", "clean") + "_out"]) for d in noisy)   # the noise flips bits at every order
    assert [s["mod"] for s in lists["spec"]] == list(MPSK_ORDERS)
    for fn, orders in (("qam_gray_encode_bb", QAM_ORDERS), ("mpsk_gray_encode_bb", MPSK_ORDERS)):
        for mod in orders:
            cases = [m for m in lists["map"] if m["fn"] == fn and m["mod"] == mod]
            bps = int(np.log2(mod))
            assert any(m["nbits"] % bps for m in cases) or bps == 1
            assert any(m["nbits"] % bps == 0 for m in cases) and all(m["n_symb"] == m["nbits"] // bps == m["data_len"] // bps for m in cases)
    assert conv22["bad order"]["qam_gray_decode mod 8"] == {"raises": "ValueError", "message": "M must be 2, 4, 16, 64, 256"}
    assert conv22["bad order"]["mpsk_gray_decode mod 64"] == {"raises": "ValueError", "message": "M must be 2, 4, 8, 16, or 32"}
    assert all(v["shape"] == [0] and v["dtype"] == "int64" for v in conv22["empty input"].values()) and len(conv22["empty input"]) == 6
    assert len(conv22["deliberate differences"]) >= 6


def test_host_forms_equal_every_captured_decode(g22):
    g, lists = g22
    for d in lists["dec"]:
        x, want = g[d["key"] + "_in"], g[d["key"] + "_out"]
        got = getattr(dc, d["fn"] + "_host")(x, d["mod"])
        assert got.dtype == want.dtype == np.dtype(d["out_dtype"]) and np.array_equal(got, want), d["key"]


def test_host_mpsk_equals_the_exact_specials(g22):
    g, lists = g22
    for s in lists["spec"]:
        x, want = g[s["key"] + "_in"], g[s["key"] + "_out"]
        assert np.array_equal(dc.mpsk_gray_decode_host(x, s["mod"]), want), s
    # the quirks the issue names: mod 2 decodes -1 to bit 1 and +1 to bit 0; 0 decodes as angle 0; -1 - 0j as +pi's index
    assert list(dc.mpsk_gray_decode_host(np.array([-1, 1, 0, complex(-1.0, -0.0)]), 2)) == [1, 0, 0, 1]


def test_host_mapper_equals_every_captured_sequence(g22):
    g, lists = g22
    for m in lists["map"]:
        kind = _ffi.QAM if m["fn"].startswith("qam") else _ffi.MPSK
        bits, want = g[m["key"] + "_bits"], g[m["key"] + "_x"]
        got = _ffi.gray_map_rows_host(bits[None, :], kind, m["mod"])
        assert got.dtype == np.complex128 and got.shape == (1, m["n_symb"]) and np.array_equal(got[0], want), m["key"]
        assert np.array_equal(got[0].view(np.float64).view(np.uint64), want.view(np.float64).view(np.uint64)) or m["mod"] == 2, m["key"]   # bit-identical
        x_own = (dc.qam_gray_encode_bb if kind == _ffi.QAM else dc.mpsk_gray_encode_bb)(None, 1, m["mod"], ext_data=bits.astype(np.int64))[0]
        assert np.array_equal(np.asarray(x_own, dtype=np.complex128), want)         # the existing encoders: unchanged
        c64 = _ffi.gray_map_rows_host(bits[None, :], kind, m["mod"], np.complex64)
        assert c64.dtype == np.complex64 and np.array_equal(c64[0], want.astype(np.complex64))


def test_conventions_that_need_no_device(conv22):
    for fn in ("qam_gray_decode", "mpsk_gray_decode"):
        assert str(inspect.signature(getattr(dc, fn))) == conv22["signatures"][fn]
        assert str(inspect.signature(getattr(dc, fn + "_host"))) == conv22["signatures"][fn]
    one = np.ones(5) + 1j * np.arange(5)
    for f in (dc.qam_gray_decode, dc.qam_gray_decode_host, dc.qam_gray_decode_rows, dc.qam_gray_map_rows):
        for x in (one, one[:0]):
            with pytest.raises(ValueError, match="^M must be 2, 4, 16, 64, 256$"):
                f(x.reshape(1, -1) if f in (dc.qam_gray_decode_rows, dc.qam_gray_map_rows) else x, 8)
    for f in (dc.mpsk_gray_decode, dc.mpsk_gray_decode_host, dc.mpsk_gray_decode_rows, dc.mpsk_gray_map_rows):
        with pytest.raises(ValueError, match="^M must be 2, 4, 8, 16, or 32$"):
            f(one.reshape(1, -1) if f in (dc.mpsk_gray_decode_rows, dc.mpsk_gray_map_rows) else one, 64)
    for f, mods in ((dc.qam_gray_decode, QAM_ORDERS), (dc.qam_gray_decode_host, QAM_ORDERS), (dc.mpsk_gray_decode, MPSK_ORDERS), (dc.mpsk_gray_decode_host, MPSK_ORDERS)):
        for mod in mods:        # empty: the reference's dtype, no launch (no library is loaded for it)
            y = f(np.zeros(0, dtype=np.complex128), mod)
            assert y.shape == (0,) and y.dtype == np.int64
    assert dc.qam_gray_decode_rows(np.zeros((3, 0), dtype=np.complex64), 16).shape == (3, 0)
    assert dc.mpsk_gray_decode_rows(np.zeros((2, 4)), 8, start=4).shape == (2, 0)
    with pytest.raises(ValueError, match="zero or not finite"):
        dc.qam_gray_decode_host(np.full(7, 1 + 1j), 4)
    with pytest.raises(ValueError, match="zero or not finite"):
        dc.qam_gray_decode_host(np.array([1, -1, np.inf, 1j]), 4)
    with pytest.raises(ValueError, match="one-dimensional"):
        dc.qam_gray_decode_host(np.zeros((2, 2)), 4)
    with pytest.raises(ValueError, match="bits 0 / 1 only"):
        dc.qam_gray_map_rows(np.array([[0, 2, 1, 1]]), 4)
    # real, integer and single-precision input: widened to complex128, decided in float64
    xr = np.array([0.9, -1.2, 1.4, -0.7, 1.0])
    assert np.array_equal(dc.qam_gray_decode_host(xr, 2), dc.qam_gray_decode_host(xr.astype(np.complex128), 2))
    xi = np.array([3, -1, 1, -3, 1, -1])
    assert np.array_equal(dc.qam_gray_decode_host(xi, 4), dc.qam_gray_decode_host(xi.astype(np.complex128), 4))
    assert np.array_equal(dc.mpsk_gray_decode_host(xi, 2), [0, 1, 0, 1, 0, 1])
    x32 = (np.array([0.31, -0.9, 0.2]) + 1j * np.array([0.5, 0.1, -0.77])).astype(np.complex64)
    assert np.array_equal(dc.mpsk_gray_decode_host(x32, 8), dc.mpsk_gray_decode_host(x32.astype(np.complex128), 8))


# ---------------------------------------------------------------------------------------------------------------- the kernels' plan on the CPU
def build_emul(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "symmap_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("symmap"), "symmap_emul", [])


def plan_of(exe):
    words = subprocess.check_output([exe, "plan"]).decode().split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def edge_lengths(plan):
    return sorted({1, 2, 15, 16, 17, plan["run"] - 1, plan["run"], plan["run"] + 1, plan["wg"] - 1, plan["wg"], plan["wg"] + 1, 2 * plan["wg"] + 3})


def emul_map(exe, tmp, bits2d, kind, mod, dtype, n, in_off=0, out_off=0, y_stride=None):
    """bits2d: (nrow, bits_stride) bytes; the rows' first bps n bytes are the bits.  Returns (nrow, n) points."""
    c64 = np.dtype(dtype) == np.complex64
    nrow, bs = bits2d.shape
    ys = n if y_stride is None else y_stride
    bps = _ffi.sym_bits(kind, mod)
    f = [str(tmp / name) for name in ("tab.f64", "in.u8", "out.bin")]
    np.concatenate(_ffi.gray_table(kind, mod, dtype)).tofile(f[0])
    bits2d.reshape(-1)[:(nrow - 1) * bs + bps * n].tofile(f[1])
    subprocess.check_call([exe, "map", str(kind), str(mod), str(int(c64)), str(n), str(nrow), str(bs), str(ys), str(in_off), str(out_off)] + f)
    y = np.fromfile(f[2], dtype=dtype)
    return np.stack([y[r * ys:r * ys + n] for r in range(nrow)])


def span(x_stride, start, step, n, nrow):
    return (nrow - 1) * x_stride + start + (n - 1) * step + 1


def emul_scale(exe, tmp, x2d, mod, start, step, n):
    f = str(tmp / "x.bin")
    nrow, xs = x2d.shape
    x2d.reshape(-1)[:span(xs, start, step, n, nrow)].tofile(f)
    out = subprocess.check_output([exe, "scl", str(mod), str(int(x2d.dtype == np.complex64)), str(n), str(nrow), str(xs), str(start), str(step),
                                   float(_ffi.qam_scale_const(mod)).hex(), f])
    return np.array([float.fromhex(v) for v in out.decode().split()])


def emul_demap(exe, tmp, x2d, kind, mod, start, step, n, r=None, bits_stride=None, out_off=0):
    nrow, xs = x2d.shape
    bps = _ffi.sym_bits(kind, mod)
    bs = bps * n if bits_stride is None else bits_stride
    f = [str(tmp / name) for name in ("r.f64", "x.bin", "out.u8")]
    np.asarray(np.ones(nrow) if r is None else r, dtype=np.float64).tofile(f[0])
    x2d.reshape(-1)[:span(xs, start, step, n, nrow)].tofile(f[1])
    subprocess.check_call([exe, "dec", str(kind), str(mod), str(int(x2d.dtype == np.complex64)), str(n), str(nrow), str(xs), str(start), str(step), str(bs), str(out_off),
                           float(ROT.real).hex(), float(ROT.imag).hex()] + f)
    y = np.fromfile(f[2], dtype=np.uint8)
    return np.stack([y[r_ * bs:r_ * bs + bps * n] for r_ in range(nrow)])


def host_demap(x1d, kind, mod, r=None):
    """the yardstick of one row: the _host arithmetic, with the scale given (QAM)"""
    x = np.asarray(x1d).astype(np.complex128)
    return dc._qam_bits_host(x, mod, r) if kind == _ffi.QAM else dc._mpsk_bits_host(x, mod)


def symbols(rng, kind, mod, shape, dtype):
    """noisy constellation points at a random gain"""
    bps = _ffi.sym_bits(kind, mod)
    bits = rng.integers(0, 2, (int(np.prod(shape)), bps)).astype(np.uint8)
    x = _ffi.gray_map_rows_host(bits.reshape(1, -1), kind, mod)[0]
    x = (x + 0.3 / np.sqrt(mod) * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))) * 1.7
    return x.reshape(shape).astype(dtype)


def exact_scale(x1d, mod):
    """r by exact sums of the widened values: the definition, rounded once per step"""
    x = np.asarray(x1d).astype(np.complex128)
    n = x.size
    mre, mim = math.fsum(x.real) / n, math.fsum(x.imag) / n
    m2 = math.fsum((np.longdouble(x.real) - np.longdouble(mre)) ** 2) + math.fsum((np.longdouble(x.imag) - np.longdouble(mim)) ** 2)
    return 1.0 / (math.sqrt(m2 / n) * math.sqrt(3 / (2 * (mod - 1))))


def test_plan_is_what_the_kernels_document(emul):
    p = plan_of(emul)
    assert p == {"run": 8, "wg": 2048, "threads": 256} and p["wg"] == p["run"] * p["threads"]


def test_emulated_mapper_equals_the_host_form(emul, tmp_path):
    """every bits-per-symbol value, the edge lengths, both output dtypes, rows whose bits start at every byte alignment modulo 16 (three rows,
    a stride of bps n + 5, the window in_off bytes off a boundary) and whose points start on and off a 16-byte boundary"""
    rng = np.random.default_rng(221)
    plan = plan_of(emul)
    for ci, (kind, mod) in enumerate(FAMILIES):
        bps = _ffi.sym_bits(kind, mod)
        lens = edge_lengths(plan) if mod in (16, 8) else [1, 17, plan["wg"] + 1]
        for li, n in enumerate(lens):
            dtype = (np.complex64, np.complex128)[(ci + li) % 2]
            nrow = 3 if n < 3000 else 1
            bits = rng.integers(0, 2, (nrow, bps * n + 5)).astype(np.uint8)
            got = emul_map(emul, tmp_path, bits, kind, mod, dtype, n, in_off=(3 * li + ci) % 16, out_off=(li + ci) % 2, y_stride=n + 1)
            assert np.array_equal(got, _ffi.gray_map_rows_host(bits[:, :bps * n], kind, mod, dtype)), (kind, mod, n, dtype)


def test_emulated_demap_equals_the_host_form(emul, tmp_path):
    """every order, the edge lengths, start in {0, 5} and step in {1, 4, 7}, output rows at every byte alignment modulo 16, both input dtypes;
    the QAM scale is given (a power of two times a constant), so the comparison is of decisions alone"""
    rng = np.random.default_rng(222)
    plan = plan_of(emul)
    for ci, (kind, mod) in enumerate(FAMILIES):
        bps = _ffi.sym_bits(kind, mod)
        lens = edge_lengths(plan) if mod in (16, 8) else [1, 16, plan["wg"] + 1]
        for li, n in enumerate(lens):
            start, step = (0, 5)[(li + ci) % 2], (1, 4, 7)[(li + ci // 2) % 3]
            dtype = (np.complex128, np.complex64)[(ci + li) % 2]
            nrow = 3 if n < 3000 else 1
            x = symbols(rng, kind, mod, (nrow, start + n * step + 2), dtype)
            r = 1.0 / (np.std(x[:, start::step][:, :n].astype(np.complex128), axis=1) * _ffi.qam_scale_const(mod)) if kind == _ffi.QAM and n > 1 else np.full(nrow, 0.61)
            got = emul_demap(emul, tmp_path, x, kind, mod, start, step, n, r, bits_stride=bps * n + 3, out_off=(5 * li + ci) % 16)
            for row in range(nrow):
                want = host_demap(x[row, start::step][:n], kind, mod, r[row])
                assert np.array_equal(got[row], want), (kind, mod, n, start, step, row)


def test_emulated_mpsk_equals_the_exact_specials_and_fixtures(g22, emul, tmp_path):
    """the kernels' own angle (atan2_rn: + - * / and fma alone, so host and device agree to the bit) on the reference's captured decisions: the
    specials that sit ON a threshold (1, 1j, ... under the QPSK rotation), where one ulp of the angle decides, and every MPSK fixture"""
    g, lists = g22
    cases = [(s["key"], s["mod"]) for s in lists["spec"]] + [(d["key"], d["mod"]) for d in lists["dec"] if d["fn"] == "mpsk_gray_decode" and d["ref_in"] == "same"]
    for key, mod in cases:
        x, want = g[key + "_in"], g[key + "_out"]
        for dtype in (np.complex128,) + ((np.complex64,) if key.startswith("ps_") else ()):
            got = emul_demap(emul, tmp_path, x.astype(dtype)[None, :], _ffi.MPSK, mod, 0, 1, x.size)
            assert np.array_equal(got[0], want), (key, dtype)


def test_emulated_decision_on_ties_and_clipping(emul, tmp_path):
    """contract item 2 on the CPU: components exactly on k + 0.5 (r a power of two: the products are exact), far outside the constellation,
    the largest finite values, signed zeros -- qam_level against the reference's four NumPy steps, array_equal"""
    for mod in QAM_ORDERS:
        x_m = 1 if mod == 2 else int(np.sqrt(mod)) - 1
        for r in (0.25, 1.0, 8.0, 1.0 / 3.0, 0.7310585786300049):
            k = np.arange(-3, x_m + 4)
            ties = (2 * (k + 0.5) - x_m) / r if r in (0.25, 1.0, 8.0) else np.zeros(0)
            near = np.concatenate([np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf)])
            v = np.concatenate([ties, near, [0.0, -0.0, 1e300, -1e300, np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324],
                                np.random.default_rng(mod).uniform(-2 * x_m / r, 2 * x_m / r, 500)])
            fin, fout = str(tmp_path / "v.f64"), str(tmp_path / "k.i32")
            v.tofile(fin)
            subprocess.check_call([emul, "lvl", str(x_m), float(r).hex(), fin, fout])
            got = np.fromfile(fout, dtype=np.int32)
            with np.errstate(over="ignore"):
                finite = np.isfinite(v * r)
                want = np.int16(np.clip(np.rint((v * r + x_m) / 2), 0, x_m))
            assert np.array_equal(got, want), (mod, r)
            if ties.size:   # ... and those four steps ARE the reference's: x / s with s = 1 / r (exact for a power of two), a complex array like the reference's
                fin_ = v[finite]                      # (where x / s overflows the reference's complex division gives NaN, whose cast is platform-defined;
                s = 1.0 / r                           #  the kernel clips such values to the end levels)
                kk = ((fin_ + 1j * fin_) / s + x_m * (1 + 1j)) / 2
                for part in (kk.real, kk.imag):
                    assert np.array_equal(np.int16(np.clip(np.rint(part), 0, x_m)), want[finite])


def test_emulated_scale_is_accurate_and_ordered(emul, tmp_path):
    """the merge of partial moments against exact sums: 1e-13 for |mean| <= std, 1e-12 at |mean| = 1000 std; rows of one item,
    of several with a partial last one, of two symbols; strided; both dtypes (complex64 widened exactly)"""
    rng = np.random.default_rng(223)
    plan = plan_of(emul)
    for n, nrow, start, step, dtype in ((2, 1, 0, 1, np.complex128), (plan["wg"] + 1, 3, 5, 4, np.complex128), (5 * plan["wg"] + 77, 1, 0, 1, np.complex64),
                                        (2 ** 16 + 3, 1, 0, 7, np.complex128)):
        for offset in (0.0, 1000.0):
            x = symbols(rng, _ffi.QAM, 64, (nrow, start + n * step + 1), np.complex128)
            x = (x + offset * np.std(x) * np.exp(0.3j)).astype(dtype)
            got = emul_scale(emul, tmp_path, x, 64, start, step, n)
            for row in range(nrow):
                want = exact_scale(x[row, start::step][:n], 64)
                assert abs(got[row] / want - 1) <= (1e-12 if offset else 1e-13), (n, offset, row, got[row] / want - 1)


def test_sanitized_emulation_as_a_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation (its own main, run as a child process): every kernel over several work items
    with a partial last one, windows off a 16-byte boundary inside exact-size allocations, strided input whose last symbol is the allocation's
    last element (an overrun of staging or of the strided reads shows here, not on a GPU)"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "symmap_emul_san", san)
    plan = plan_of(exe)
    rng = np.random.default_rng(224)
    n = 2 * plan["wg"] + 3
    for kind, mod, dtype, off in ((_ffi.QAM, 256, np.complex64, 1), (_ffi.QAM, 64, np.complex128, 3), (_ffi.MPSK, 32, np.complex128, 15), (_ffi.MPSK, 8, np.complex64, 0),
                                  (_ffi.QAM, 2, np.complex64, 7)):
        bps = _ffi.sym_bits(kind, mod)
        bits = rng.integers(0, 2, (2, bps * n + 1)).astype(np.uint8)
        y = emul_map(exe, tmp_path, bits, kind, mod, dtype, n, in_off=off, out_off=off % 2, y_stride=n + 1)
        assert np.array_equal(y, _ffi.gray_map_rows_host(bits[:, :bps * n], kind, mod, dtype))
        x = symbols(rng, kind, mod, (2, 5 + n * 4), dtype)
        r = emul_scale(exe, tmp_path, x, mod, 5, 4, n) if kind == _ffi.QAM else None
        got = emul_demap(exe, tmp_path, x, kind, mod, 5, 4, n, r, bits_stride=bps * n + 1, out_off=off)
        for row in range(2):
            assert np.array_equal(got[row], host_demap(x[row, 5::4][:n], kind, mod, None if r is None else r[row]))
