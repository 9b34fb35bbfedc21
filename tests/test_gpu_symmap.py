"""Gray symbol mapping and demapping on the GPU (csrc/symmap.hip) against the NumPy yardsticks (digitalcom.*_host, _ffi.gray_map_rows_host) and
the fixtures captured from the real reference (g22_symmap.npz).  The contract is DESIGN.md 4.17's: the mapper and the decision with a given
scale compare by array_equal for every input; the scale is within 1e-13 (|mean| <= std) resp. 1e-12 (|mean| = 1000 std) of an exact evaluation
and identical from run to run; end to end every fixture (whose least margin from a threshold the generator guarantees) compares by
array_equal with no symbol excluded."""
import ctypes

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc
from test_symmap_cpu import FAMILIES, MPSK_ORDERS, QAM_ORDERS, exact_scale, g22, host_demap, symbols  # noqa: F401  (g22: the fixture)

pytestmark = pytest.mark.gpu

RUN, WG = 8, 2048                      # symbols per lane / per work item (test_symmap_cpu asserts them against the core header)
LENGTHS = (1, 2, 15, 16, 17, RUN - 1, RUN, RUN + 1, WG - 1, WG, WG + 1, 2 * WG + 3)
SENTINEL = 0xA5


def _c(dtype):
    return np.dtype(dtype).itemsize


def dev_map(bits2d, kind, mod, dtype, in_off, out_off):
    """bits2d: (nrow, bps n) -> the rows through gray_map_rows_dev: the bits in_off bytes into a device block, rows bps n + 5 bytes apart; the
    points out_off elements into a sentinel-filled block, rows n + 1 elements apart.  Returns (points, the whole output block)."""
    bps = _ffi.sym_bits(kind, mod)
    nrow, n = bits2d.shape[0], bits2d.shape[1] // bps
    bs, ys = bps * n + 5, n + 1
    src = np.full(in_off + nrow * bs, 0xFF, dtype=np.uint8)
    for r in range(nrow):
        src[in_off + r * bs:in_off + r * bs + bps * n] = bits2d[r]
    b = _ffi.DeviceBytes(src.size)
    b.write(src)
    total = out_off + nrow * ys + 3
    y = _ffi.DeviceBytes(total * _c(dtype))
    y.write(np.full(total * _c(dtype), SENTINEL, dtype=np.uint8))
    _ffi.gray_map_rows_dev(b.ptr + in_off, bs, n, nrow, kind, mod, dtype, y.ptr + out_off * _c(dtype), ys)
    raw = y.read()
    b.free()
    y.free()
    pts = raw.view(dtype)
    return np.stack([pts[out_off + r * ys:out_off + r * ys + n] for r in range(nrow)]), raw, [(out_off + r * ys) * _c(dtype) for r in range(nrow)]


@pytest.mark.parametrize("kind,mod", FAMILIES)
def test_mapper_equals_the_table_lookup(kind, mod):
    """every order, 1 and 3 rows, the edge lengths, both output dtypes, the bits at odd byte offsets, the points on and off a 16-byte boundary;
    nothing outside the rows' points is written"""
    _ffi.init()
    rng = np.random.default_rng(300 + mod + kind)
    bps = _ffi.sym_bits(kind, mod)
    for li, n in enumerate(LENGTHS):
        for nrow in (1, 3):
            for dtype in (np.complex64, np.complex128):
                bits = rng.integers(0, 2, (nrow, bps * n)).astype(np.uint8)
                _ffi.debug_path()
                got, raw, firsts = dev_map(bits, kind, mod, dtype, in_off=(1, 3, 7, 13)[li % 4], out_off=(li + nrow) % 2)
                assert _ffi.debug_path() == ["symmap"]
                want = _ffi.gray_map_rows_host(bits, kind, mod, dtype)
                assert got.dtype == want.dtype and np.array_equal(got, want), (n, nrow, dtype)
                keep = np.ones(raw.size, dtype=bool)
                for f in firsts:
                    keep[f:f + n * _c(dtype)] = False
                assert np.all(raw[keep] == SENTINEL), (n, nrow, dtype)


def test_mapper_equals_every_captured_sequence(g22):
    g, lists = g22
    for m in lists["map"]:
        fn = dc.qam_gray_map_rows if m["fn"].startswith("qam") else dc.mpsk_gray_map_rows
        bits, want = g[m["key"] + "_bits"], g[m["key"] + "_x"]
        got = fn(np.stack([bits, 1 - bits]), m["mod"])
        assert got.dtype == np.complex128 and got.shape == (2, m["n_symb"]) and np.array_equal(got[0], want), m["key"]
        assert np.array_equal(fn(bits[None, :], m["mod"], np.complex64)[0], want.astype(np.complex64)), m["key"]


@pytest.mark.parametrize("mod", QAM_ORDERS)
def test_decision_with_a_given_scale_is_the_reference_arithmetic(mod):
    """contract item 2: components exactly on k + 0.5 (r a power of two, so the products are exact, in complex64 as well), their float
    neighbours, values far outside the constellation and random ones; every start / step; both dtypes -- array_equal with the four steps"""
    _ffi.init()
    rng = np.random.default_rng(400 + mod)
    x_m = 1 if mod == 2 else int(np.sqrt(mod)) - 1
    for ci, (start, step) in enumerate(((0, 1), (5, 4), (0, 7), (5, 1))):
        for dtype in (np.complex128, np.complex64):
            r = (0.25, 8.0, 1.0, 0.5)[ci]
            real = np.float32 if dtype == np.complex64 else np.float64
            k = np.arange(-3, x_m + 4)
            ties = ((2 * (k + 0.5) - x_m) / r).astype(real)
            pool = np.concatenate([ties, np.nextafter(ties, real(np.inf)), np.nextafter(ties, real(-np.inf)), [0.0, -0.0, 1e30, -1e30, 3e38, -3e38],
                                   rng.uniform(-2 * x_m / r, 2 * x_m / r, 64).astype(real)]).astype(np.float64)
            n = 2 * WG + 3
            x = np.zeros((3, start + (n - 1) * step + 1), dtype=dtype)
            x.real = rng.choice(pool, x.shape)
            x.imag = rng.choice(pool, x.shape)
            rr = np.array([r, r * 2, r / 4])
            got = _ffi.gray_demap_rows(x, _ffi.QAM, mod, start, step, rr)
            for row in range(3):
                assert np.array_equal(got[row], host_demap(x[row, start::step][:n], _ffi.QAM, mod, rr[row])), (mod, start, step, dtype, row)


@pytest.mark.parametrize("nrow,n", [(1, 2 ** 20 + 3), (3, WG + 1), (1, 2)])
def test_scale_is_accurate_and_repeats(nrow, n):
    """contract item 3: against exact sums of the same definition, 1e-13 for |mean| <= std, 1e-12 at |mean| = 1000 std; two runs, the same bits"""
    _ffi.init()
    rng = np.random.default_rng(500 + n % 97)
    for offset in (0.0, 1000.0):
        for dtype in (np.complex128, np.complex64) if n < 2 ** 20 else (np.complex128,):
            x = symbols(rng, _ffi.QAM, 64, (nrow, n), np.complex128)
            x = (x + offset * np.std(x) * np.exp(0.3j)).astype(dtype)
            _ffi.debug_path()
            r1 = _ffi.qam_scale_rows(x, 64)
            assert _ffi.debug_path() == ["symscale"]
            r2 = _ffi.qam_scale_rows(x, 64)
            assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
            for row in range(nrow):
                err = abs(r1[row] / exact_scale(x[row], 64) - 1)
                print("scale n = %d rows = %d offset = %g %s: relative error %.3g" % (n, nrow, offset, np.dtype(dtype).name, err))
                assert err <= (1e-12 if offset else 1e-13), (n, offset, dtype, row, err)


def test_public_functions_equal_every_captured_decode(g22):
    """contract items 4 - 6 through the public functions and the _rows forms: array_equal, the reference's dtype, no symbol excluded"""
    g, lists = g22
    for d in lists["dec"]:
        x, want = g[d["key"] + "_in"], g[d["key"] + "_out"]
        _ffi.debug_path()
        got = getattr(dc, d["fn"])(x, d["mod"])
        assert _ffi.debug_path() == (["symscale", "symdemap"] if d["fn"].startswith("qam") else ["symdemap"])
        assert got.dtype == want.dtype and np.array_equal(got, want), d["key"]
        rows = getattr(dc, d["fn"] + "_rows")(np.stack([x, 4 * x]) + 0j, d["mod"])       # a gain (exact here) does not matter: each row has its own np.std
        assert rows.dtype == np.uint8 and np.array_equal(rows[0], want) and np.array_equal(rows[1], want), d["key"]
    for s in lists["spec"]:
        x, want = g[s["key"] + "_in"], g[s["key"] + "_out"]
        assert np.array_equal(dc.mpsk_gray_decode(x, s["mod"]), want), s
        assert np.array_equal(dc.mpsk_gray_decode(x.astype(np.complex64), s["mod"]), want), s
    assert list(dc.mpsk_gray_decode(np.array([-1, 1, 0, complex(-1.0, -0.0)]), 2)) == [1, 0, 0, 1]


@pytest.mark.parametrize("kind,mod", FAMILIES)
def test_rows_forms_equal_the_host_forms(kind, mod):
    """three frames at different gains and offsets behind a matched filter's stride: every row equals the 1-D function and the _host form"""
    rng = np.random.default_rng(600 + mod + kind)
    name = "qam_gray_decode" if kind == _ffi.QAM else "mpsk_gray_decode"
    for start, step, n, dtype in ((0, 1, WG + 1, np.complex128), (5, 4, 2 * WG + 3, np.complex64), (5, 7, 17, np.complex128)):
        x = symbols(rng, kind, mod, (3, start + (n - 1) * step + 1), np.complex128)
        x = (x * np.array([[0.3], [1.0], [40.0]]) + np.array([[0.0], [0.01], [-0.2j]])).astype(dtype)
        for row in range(3):        # the generator's margin rule, applied to the inputs drawn here: no threshold nearer than 1e-6 level / index units
            frame = x[row, start::step][:n].astype(np.complex128)
            if kind == _ffi.QAM:
                xm = 1 if mod == 2 else np.sqrt(mod) - 1
                kk = (frame * dc._qam_scale_host(frame, mod) + xm * (1 + 1j)) / 2
                parts = np.concatenate([kk.real, kk.imag if mod > 2 else kk.real])
                parts = parts[(parts > 0) & (parts < xm)]
            else:
                parts = np.angle(frame * (np.exp(-1j * np.pi / 4) if mod == 4 else 1)) * mod / 2 / np.pi
            assert np.min(np.abs(np.abs(parts - np.floor(parts)) - 0.5)) >= 1e-6, "the drawn input is ambiguous: draw another"
        got = getattr(dc, name + "_rows")(x, mod, start, step)
        assert got.dtype == np.uint8 and got.shape == (3, n * _ffi.sym_bits(kind, mod))
        for row in range(3):
            frame = x[row, start::step][:n]
            assert np.array_equal(got[row], getattr(dc, name + "_host")(frame, mod)), (start, step, row)
            assert np.array_equal(got[row], getattr(dc, name)(frame, mod)), (start, step, row)


def test_all_equal_row_raises():
    x = symbols(np.random.default_rng(7), _ffi.QAM, 16, (3, 40), np.complex128)
    x[1, :] = 0.5 - 0.25j
    with pytest.raises(ValueError, match="zero or not finite"):
        dc.qam_gray_decode_rows(x, 16)
    with pytest.raises(ValueError, match="zero or not finite"):
        dc.qam_gray_decode(x[1], 16)
    x[1, 3] = np.nan
    with pytest.raises(ValueError, match="zero or not finite"):
        dc.qam_gray_decode_rows(x, 16)


@pytest.mark.parametrize("kind,mod", [(_ffi.QAM, 16), (_ffi.MPSK, 8)])
def test_device_resident_round_trip(kind, mod):
    """bits -> gray_map_rows_dev -> qam_scale_rows_dev -> gray_demap_rows_dev -> bit_count_rows_dev on 5 rows of 2 WG + 3 symbols with no host
    copy between the stages: every count is 0; with one symbol per row replaced by a neighbour of the constellation, each row's count is that
    row's host-computed Hamming distance"""
    _ffi.init()
    rng = np.random.default_rng(700 + mod)
    bps, nrow, n = _ffi.sym_bits(kind, mod), 5, 2 * WG + 3
    bits = rng.integers(0, 2, (nrow, bps * n)).astype(np.uint8)
    tx, rx, cnt, r = _ffi.DeviceBytes(bits.size), _ffi.DeviceBytes(bits.size), _ffi.DeviceBytes(8 * nrow), _ffi.DeviceBytes(8 * nrow)
    tx.write(bits.reshape(-1))
    xd = _ffi.DeviceArray(nrow * n, np.complex128)

    def chain():
        if kind == _ffi.QAM:
            _ffi.qam_scale_rows_dev(xd.ptr, n, 0, 1, n, nrow, np.complex128, mod, r.ptr)
        _ffi.gray_demap_rows_dev(xd.ptr, n, 0, 1, n, nrow, np.complex128, kind, mod, rx.ptr, r_ptr=r.ptr)
        _ffi.bit_count_rows_dev(tx.ptr, bps * n, rx.ptr, bps * n, bps * n, nrow, False, cnt.ptr)
        return cnt.read().view(np.int64)

    _ffi.debug_path()
    _ffi.gray_map_rows_dev(tx.ptr, bps * n, n, nrow, kind, mod, np.complex128, xd.ptr)
    assert np.array_equal(chain(), np.zeros(nrow, dtype=np.int64))
    assert _ffi.debug_path() == ["symmap"] + (["symscale"] if kind == _ffi.QAM else []) + ["symdemap", "bitcount"]
    # a neighbour: the next level of the in-phase component (QAM), the next phase (MPSK), computed from the points themselves
    x = _ffi.gray_map_rows_host(bits, kind, mod)
    want = np.zeros(nrow, dtype=np.int64)
    for row in range(nrow):
        p = int(rng.integers(0, n))
        if kind == _ffi.QAM:
            lv = np.unique(x.real)
            i = int(np.argmin(np.abs(lv - x[row, p].real)))
            x[row, p] = lv[i + 1 if i + 1 < lv.size else i - 1] + 1j * x[row, p].imag
        else:
            x[row, p] = x[row, p] * np.exp(2j * np.pi / mod)
        xd.write(x[row, p:p + 1], row * n + p)
        want[row] = int(np.sum(getattr(dc, ("qam" if kind == _ffi.QAM else "mpsk") + "_gray_decode_host")(x[row], mod) != bits[row]))
    assert np.all(want >= 1) and np.array_equal(chain(), want)
    for d in (tx, rx, cnt, r, xd):
        d.free()


@pytest.mark.parametrize("kind,mod,dtype", [(_ffi.QAM, 64, np.complex64), (_ffi.QAM, 16, np.complex128), (_ffi.MPSK, 8, np.complex64), (_ffi.MPSK, 32, np.complex128)])
def test_input_footprint(kind, mod, dtype):
    """the scale and demap kernels read x[row, start + k step], k < n, and nothing else: the elements in front of the first symbol, between the
    symbols, behind the last one of every row and around the whole block are filled with zeros, then with finite values that would change every
    row's np.std (and with it the decisions) or turn the angles if one were read -- the scales and the bits must be the same bytes"""
    _ffi.init()
    rng = np.random.default_rng(800 + mod)
    bps, nrow, n, start, step, pad = _ffi.sym_bits(kind, mod), 3, WG + 5, 5, 4, 4096
    width = start + n * step + 3
    sym = symbols(rng, kind, mod, (nrow, n), dtype)
    outs = []
    for fill in (0.0, -997.0 + 1531.0j):
        block = np.full(2 * pad + nrow * width, fill, dtype=dtype)
        rows = block[pad:pad + nrow * width].reshape(nrow, width)
        rows[:, start:start + n * step:step] = sym
        xd = _ffi.DeviceArray.from_host(block)
        x_ptr = xd.ptr + pad * _c(dtype)
        r, out = _ffi.DeviceBytes(8 * nrow), _ffi.DeviceBytes(nrow * bps * n)
        if kind == _ffi.QAM:
            _ffi.qam_scale_rows_dev(x_ptr, width, start, step, n, nrow, dtype, mod, r.ptr)
        _ffi.gray_demap_rows_dev(x_ptr, width, start, step, n, nrow, dtype, kind, mod, out.ptr, r_ptr=r.ptr)
        outs.append((r.read() if kind == _ffi.QAM else None, out.read()))
        for d in (xd, r, out):
            d.free()
    if kind == _ffi.QAM:
        assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    want = np.stack([host_demap(sym[row], kind, mod, None if kind == _ffi.MPSK else outs[0][0].view(np.float64)[row]) for row in range(nrow)])
    assert np.array_equal(outs[0][1].reshape(nrow, -1), want)


def test_refusals_by_message():
    _ffi.init()
    x = _ffi.DeviceArray(64, np.complex128)
    b = _ffi.DeviceBytes(1024)
    with pytest.raises(ValueError, match="M must be 2, 4, 16, 64, 256"):
        _ffi.check(_ffi.load().skdsp_qam_scale_rows_dev(ctypes.c_void_p(x.ptr), 64, 0, 1, 64, 1, _ffi.C128, 8, 1.0, ctypes.c_void_p(b.ptr)))
    with pytest.raises(ValueError, match="complex64 or complex128"):
        _ffi.check(_ffi.load().skdsp_mpsk_demap_rows_dev(ctypes.c_void_p(x.ptr), 64, 0, 1, 64, 1, _ffi.F64, 8, 1.0, 0.0, ctypes.c_void_p(b.ptr), 192))
    with pytest.raises(ValueError, match="aligned"):
        _ffi.check(_ffi.load().skdsp_mpsk_demap_rows_dev(ctypes.c_void_p(x.ptr + 8), 32, 0, 1, 32, 1, _ffi.C128, 8, 1.0, 0.0, ctypes.c_void_p(b.ptr), 96))
    with pytest.raises(ValueError, match="step"):
        _ffi.check(_ffi.load().skdsp_mpsk_demap_rows_dev(ctypes.c_void_p(x.ptr), 64, 0, 0, 64, 1, _ffi.C128, 8, 1.0, 0.0, ctypes.c_void_p(b.ptr), 192))
    x.free()
    b.free()


@pytest.mark.parametrize("nrow,width,start,step", [(1, 1, 0, 1), (3, 77, 0, 1), (2, 301, 2, 3)])
def test_qam_scale_host_form_equals_the_device_form(nrow, width, start, step):
    """skdsp_qam_scale_rows (host pointers: the rows are staged whole, the scales come back) against skdsp_qam_scale_rows_dev, bit for bit"""
    rng = np.random.default_rng(65 + width)
    for dtype in (np.complex64, np.complex128):
        x = (rng.standard_normal((nrow, width)) + 1j * rng.standard_normal((nrow, width)) + (0.5 if width == 1 else 0)).astype(dtype)
        n = _ffi.sym_count(width, start, step)
        r = _ffi.qam_scale_rows(x, 16, start, step)
        xd, rd = _ffi.DeviceArray.from_host(x.reshape(-1)), _ffi.DeviceArray(nrow, np.float64)
        _ffi.qam_scale_rows_dev(xd.ptr, width, start, step, n, nrow, dtype, 16, rd.ptr)
        assert r.shape == (nrow,) and np.array_equal(rd.to_host().view(np.uint64), r.view(np.uint64)), (dtype, r)
