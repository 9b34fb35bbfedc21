"""The FEC chain around the Viterbi decoder on the MI355X (csrc/convcode.hip): every case captured from the real reference (g21) through
the rows forms and digitalcom.bit_errors, the encoder's edges (lengths read from the plan) against conv_encoder, many rows at an odd
length, state carry, puncture / depuncture over every element width and row-length edge, the count against NumPy, *_dev calls on
unaligned windows of larger device buffers, a many-workgroup case run twice, the whole chain through viterbi_decoder_rows, and the C ABI's
argument errors.  Everything is bits or element moves: every comparison is array_equal, nothing has a tolerance and nothing asserts a time."""
import ctypes
import warnings

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc, fec_conv as fc
from test_fecchain_cpu import (EDGE_CODES, PATTERNS, caught, code_of, conv21, edge_lengths, emul, g21, gather_row_lengths, host_gather_rows,  # noqa: F401  (fixtures)
                               host_rows, plan_of, random_state, unequal)

pytestmark = pytest.mark.gpu


def guard_bytes(n):
    return ((np.arange(n) * 37 + 11) % 251 + 2).astype(np.uint8)      # never 0 / 1


# ---------------------------------------------------------------------------------------------------------------- the captured cases
def test_every_reference_encoder_case_as_a_one_row_call(g21):
    g, cases = g21
    for c in cases["enc"]:
        _ffi.debug_path()
        y, s = code_of(c["G"]).conv_encoder_rows(g[c["key"] + "_in"][None], c["state"])
        assert _ffi.debug_path() == ["convenc"], c["key"]
        assert y.dtype == np.float64 and y.shape == (1, len(c["G"]) * c["n"]) and np.array_equal(y[0], g[c["key"] + "_out"]), c["key"]
        assert s == [c["state_out"]], c["key"]


def test_every_reference_puncture_case_as_a_one_row_call(g21):
    g, cases = g21
    cc = code_of(('111', '101'))
    for c in cases["punct"]:
        pat = tuple(c["pattern"])
        x = g[c["key"] + "_in"].astype(np.float64)[None] if c["key"] + "_in" in g.files else np.zeros((1, c["n"]))
        fn = (lambda: cc.puncture_rows(x, pat)) if c["fn"] == "puncture" else (lambda: cc.depuncture_rows(x, pat, c["erase_value"]))
        _ffi.debug_path()
        if unequal(pat):      # the reference's puncture fails on it from one period on; the rows forms refuse it outright
            with pytest.raises(ValueError):
                fn()
            assert _ffi.debug_path() == []
            continue
        y, w = caught(fn)
        ref = g[c["key"] + "_out"]
        assert _ffi.debug_path() == ([c["fn"]] if ref.size else []), c["key"]
        assert w == c["warnings"], c["key"]
        assert str(y.dtype) == c["out_dtype"] and y.shape == (1, ref.size) and np.array_equal(y[0], ref), c["key"]


def test_every_reference_bit_errors_case(g21):
    g, cases = g21
    for c in cases["ber"]:
        tx, rx = g[c["key"] + "_tx"], g[c["key"] + "_rx"]
        _ffi.debug_path()
        count, errors = dc.bit_errors(tx, tx if c["same"] else rx, c["n_corr"], c["n_transient"])
        assert _ffi.debug_path() == ["bitcount"], c["key"]
        assert (count, int(errors)) == (c["count"], c["errors"]) and [type(count).__name__, type(errors).__name__] == c["types"], c["key"]
    c = cases["ber"][3]      # the streams already on the device: the same answer
    tx, rx = g[c["key"] + "_tx"], g[c["key"] + "_rx"]
    dt, dr = _ffi.DeviceBytes(tx.size), _ffi.DeviceBytes(rx.size)
    dt.write(tx)
    dr.write(rx)
    count, errors = dc.bit_errors(dt, dr, c["n_corr"], c["n_transient"])
    assert (count, int(errors)) == (c["count"], c["errors"]) and type(errors) is np.int64
    assert dc.bit_errors(dt, dt, c["n_corr"], c["n_transient"]) == (tx.size - c["n_transient"], 0)


# ---------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("G", EDGE_CODES, ids=lambda G: "-".join(G))
def test_encoder_edges_equal_conv_encoder(G, emul):
    cc, K = code_of(G), len(G[0])
    rng = np.random.default_rng(K * 100 + len(G))
    for n in edge_lengths(K, plan_of(emul)):
        for state in ('1' * (K - 1), random_state(rng, K)):
            bits = rng.integers(0, 2, (1, n))
            _ffi.debug_path()
            y, s = cc.conv_encoder_rows(bits, state)
            assert _ffi.debug_path() == ["convenc"]
            ref, sref = host_rows(cc, bits, [state])
            assert y.dtype == np.float64 and np.array_equal(y, ref) and s == sref, (G, n, state)


@pytest.mark.parametrize("nrow", [1, 3, 65])
def test_rows_at_an_odd_length_with_one_state_per_row(nrow):
    for G in (('1111001', '1011011'), ('11110111', '11011001', '10010101')):
        cc, K = code_of(G), len(G[0])
        rng = np.random.default_rng(nrow)
        bits = rng.integers(0, 2, (nrow, 4099))
        states = [random_state(rng, K) for _ in range(nrow)]
        y, s = cc.conv_encoder_rows(bits, states)
        ref, sref = host_rows(cc, bits, states)
        assert np.array_equal(y, ref) and s == sref, (G, nrow)
        y1, s1 = cc.conv_encoder_rows(bits, states[0])      # one state for all rows
        ref1, sref1 = host_rows(cc, bits, [states[0]])
        assert np.array_equal(y1, ref1) and s1 == sref1
        y0, s0 = cc.conv_encoder_rows(bits)                 # rest
        assert np.array_equal(y0, host_rows(cc, bits, ['0' * (K - 1)])[0])


def test_state_carry_over_pieces_equals_one_call():
    for G in (('111', '101'), ('111101011', '101110001'), ('11110111', '11011001', '10010101')):
        cc, K = code_of(G), len(G[0])
        bits = np.random.default_rng(K).integers(0, 2, (1, 9000))
        whole, s_whole = cc.conv_encoder_rows(bits, '1' * (K - 1))
        state, parts = '1' * (K - 1), []
        for lo, hi in ((0, 1), (1, 17), (17, 9000)):
            y, s = cc.conv_encoder_rows(bits[:, lo:hi], state)
            parts.append(y)
            state = s[0]
        assert np.array_equal(np.concatenate(parts, axis=1), whole) and [state] == s_whole


# ---------------------------------------------------------------------------------------------------------------- puncture / depuncture
@pytest.mark.parametrize("pat", PATTERNS, ids=lambda p: p[0])
def test_puncture_and_depuncture_rows_equal_the_host_methods(pat):
    cc = code_of(('111', '101'))
    rng = np.random.default_rng(len(pat[0]))
    for dep in (False, True):
        name = "depuncture" if dep else "puncture"
        for n in gather_row_lengths(pat, dep) + [3 * 1024 + 7]:
            for dt in (np.uint8, np.int16, np.float32, np.float64):
                x = rng.integers(0, 60, (3, n)).astype(dt)
                _ffi.debug_path()
                if dep:
                    y, w = caught(lambda: cc.depuncture_rows(x, pat, -2.25))
                    wref = caught(lambda: cc.depuncture(x[0], pat, -2.25))[1]
                    assert y.dtype == np.float64
                    raw = _ffi.depuncture_rows(x, pat, 3.5)      # the element type kept: what the decoder's device formats use
                    assert raw.dtype == dt and np.array_equal(raw, host_gather_rows(cc, True, x.astype(np.float64), pat, float(np.array([3.5]).astype(dt)[0])))
                else:
                    y, w = caught(lambda: cc.puncture_rows(x, pat))
                    wref = caught(lambda: cc.puncture(x[0], pat))[1]
                    assert y.dtype == dt
                ref = host_gather_rows(cc, dep, x, pat, -2.25)
                assert _ffi.debug_path() == ([name] if ref.size else []), (pat, dep, n, dt)
                assert w == wref and y.shape == ref.shape and np.array_equal(y, ref), (pat, dep, n, dt)


def test_int16_erasure_is_written_as_3():
    y = _ffi.depuncture_rows(np.arange(1, 9, dtype=np.int16)[None], ('110', '101'), 3.5)
    assert y.dtype == np.int16 and y.tolist() == [[1, 2, 3, 3, 3, 4, 5, 6, 7, 3, 3, 8]]


# ---------------------------------------------------------------------------------------------------------------- count
def test_bit_count_rows_equals_numpy():
    rng = np.random.default_rng(5)
    for n in (0, 1, 15, 16, 17, 65539):
        for nrow in (1, 5):
            tx, rx = rng.integers(0, 2, (nrow, n + 9), dtype=np.uint8), rng.integers(0, 2, (nrow, n + 2), dtype=np.uint8)      # unequal strides
            for invert in (False, True):
                _ffi.debug_path()
                got = _ffi.bit_count_rows(tx, rx, invert, n)
                assert _ffi.debug_path() == (["bitcount"] if n else [])
                assert got.dtype == np.int64 and np.array_equal(got, np.sum((tx[:, :n] ^ rx[:, :n]) ^ int(invert), axis=1)), (n, nrow, invert)
    n, errs = dc.bit_errors_rows(tx, rx)
    assert n == 65541 and np.array_equal(errs, np.sum(tx[:, :n] ^ rx, axis=1))


# ---------------------------------------------------------------------------------------------------------------- device windows
OFFSETS = ((1, 3), (3, 15), (15, 1))


def window_in(data, off, pad=64):
    """data (bytes) `off` bytes behind a 256-byte aligned pad of 0xFF, 0xFF behind it: (DeviceBytes, pointer to the window)"""
    d = _ffi.DeviceBytes(data.size + 2 * pad + 16)
    host = np.full(d.nbytes, 0xFF, dtype=np.uint8)
    host[pad + off:pad + off + data.size] = data
    d.write(host)
    return d, d.ptr + pad + off


def window_out(nbytes, off, pad=64):
    d = _ffi.DeviceBytes(nbytes + 2 * pad + 16)
    guard = guard_bytes(d.nbytes)
    d.write(guard)

    def check(ref):
        got = d.read()
        lo, hi = pad + off, pad + off + nbytes
        assert np.array_equal(got[lo:hi], ref.view(np.uint8).reshape(-1))
        assert np.array_equal(got[:lo], guard[:lo]) and np.array_equal(got[hi:], guard[hi:])
        d.free()
    return d.ptr + pad + off, check


def test_device_windows_of_the_encoder_at_unaligned_offsets(emul):
    wg = plan_of(emul)["wg"]
    rng = np.random.default_rng(41)
    for G in (('1111001', '1011011'), ('11110111', '11011001', '10010101')):
        cc, K, R = code_of(G), len(G[0]), len(G)
        bits = rng.integers(0, 2, (3, wg + 5), dtype=np.uint8)
        states = [random_state(rng, K) for _ in range(3)]
        ref, sref = host_rows(cc, bits, states)
        st_in = np.array([int(s, 2) for s in states], dtype=np.uint8)
        for in_off, out_off in OFFSETS:
            din, pin = window_in(bits.reshape(-1), in_off)
            dst, pst = window_in(st_in, out_off)
            pout, check = window_out(ref.size, out_off)
            psout, check_s = window_out(3, in_off)
            _ffi.debug_path()
            cc._encoder().encode_rows_dev(pin, bits.shape[1], 3, pst, 3, pout, psout)
            assert _ffi.debug_path() == ["convenc"]
            check(ref.astype(np.uint8))
            check_s(np.array([int(s, 2) for s in sref], dtype=np.uint8))
            din.free()
            dst.free()


def test_device_windows_of_the_gathers_and_the_count_at_unaligned_offsets():
    cc = code_of(('111', '101'))
    rng = np.random.default_rng(42)
    for pat in (('110', '101'), ('1001011', '1110100')):
        for dep in (False, True):
            x = rng.integers(0, 2, (3, 2 * 1024 + 37), dtype=np.uint8)
            ref = host_gather_rows(cc, dep, x, pat, 9).astype(np.uint8)
            for in_off, out_off in OFFSETS:
                din, pin = window_in(x.reshape(-1), in_off)
                pout, check = window_out(ref.size, out_off)
                _ffi.debug_path()
                if dep:
                    _ffi.depuncture_rows_dev(pin, x.shape[1], 3, np.uint8, pat, 9, pout)
                else:
                    _ffi.puncture_rows_dev(pin, x.shape[1], 3, 1, pat, pout)
                assert _ffi.debug_path() == ["depuncture" if dep else "puncture"]
                check(ref)
                din.free()
    x = rng.integers(-40, 40, (2, 131)).astype(np.int16)      # 2-byte elements 2 bytes off a 16-byte boundary
    ref = host_gather_rows(cc, True, x.astype(np.float64), ('110', '101'), 3).astype(np.int16)
    din, pin = window_in(x.reshape(-1).view(np.uint8), 2)
    pout, check = window_out(ref.nbytes, 6)
    _ffi.depuncture_rows_dev(pin, x.shape[1], 2, np.int16, ('110', '101'), 3.5, pout)
    check(ref)
    din.free()
    n = 4096 + 19
    tx, rx = rng.integers(0, 2, (3, n + 5), dtype=np.uint8), rng.integers(0, 2, (3, n), dtype=np.uint8)
    want = np.sum(tx[:, :n] ^ rx, axis=1).astype(np.int64)
    for t_off, r_off in OFFSETS:
        dtx, ptx = window_in(tx.reshape(-1), t_off)
        drx, prx = window_in(rx.reshape(-1), r_off)
        pcnt, check = window_out(24, 8)      # (the counts: 8-byte aligned)
        _ffi.debug_path()
        _ffi.bit_count_rows_dev(ptx, n + 5, prx, n, n, 3, False, pcnt)
        assert _ffi.debug_path() == ["bitcount"]
        check(want)
        dtx.free()
        drx.free()


# ---------------------------------------------------------------------------------------------------------------- many workgroups, twice
@pytest.mark.parametrize("shape", [(1, 2 ** 20), (257, 4099)], ids=["one_row", "257_rows"])
def test_many_workgroups_twice_and_against_the_host(shape):
    cc = code_of(('1111001', '1011011'))
    bits = np.random.default_rng(shape[0]).integers(0, 2, shape, dtype=np.uint8)
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2):
            code, states = cc.conv_encoder_rows(bits, '101101')
            sent = cc.puncture_rows(code, ('110', '101'))
            back = cc.depuncture_rows(sent, ('110', '101'), 3.5)
            runs.append((code, states, sent, back))
        ref_code, ref_states = host_rows(cc, bits, ['101101'])
        ref_sent = host_gather_rows(cc, False, ref_code, ('110', '101'))
        ref_back = host_gather_rows(cc, True, ref_sent, ('110', '101'), 3.5)
    for code, states, sent, back in runs:
        assert np.array_equal(code, ref_code) and states == ref_states and np.array_equal(sent, ref_sent) and np.array_equal(back, ref_back)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]) if isinstance(a, np.ndarray))


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_the_whole_chain_decodes_what_was_sent(caplog):
    cc = fc.FECConv(('1111001', '1011011'), 35)
    bits = np.random.default_rng(7).integers(0, 2, (64, 1200))
    code, _ = cc.conv_encoder_rows(bits)
    sent = cc.puncture_rows(code, ('110', '101'))
    got = cc.viterbi_decoder_rows(cc.depuncture_rows(7.0 * sent, ('110', '101'), 3.5), 'soft', 3)      # levels 0 / 7
    assert got.shape == (64, 1200 - 34) and np.array_equal(got, bits[:, :1200 - 34])
    n, errs = dc.bit_errors_rows(bits, got)
    assert n == 1200 - 34 and errs.dtype == np.int64 and not errs.any()
    rx = 7.0 * code      # unpunctured, one received value per row at the opposite level
    where = np.random.default_rng(8).integers(0, rx.shape[1], 64)
    rx[np.arange(64), where] = 7.0 - rx[np.arange(64), where]
    got = cc.viterbi_decoder_rows(rx, 'soft', 3)
    assert np.array_equal(got, bits[:, :1200 - 34]) and not dc.bit_errors_rows(bits, got)[1].any()
    with caplog.at_level("INFO", logger=dc.log.name):
        count, errors = dc.bit_errors(bits[0, :1200 - 34], 1 - got[0])      # the decoded row inverted: found as kmax = 1, no errors
    assert (count, int(errors)) == (1200 - 34, 0) and [r.getMessage() for r in caplog.records if r.name == dc.log.name] == ['kmax =  1, taumax = 0']


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors_come_back_without_a_launch():
    L = _ffi.load()
    buf = _ffi.DeviceBytes(256)
    p = lambda off=0: ctypes.c_void_p(buf.ptr + off)      # noqa: E731
    enc = code_of(('111', '101'))._encoder()
    vit = fc.FECConv(('111', '101'), 10)._kernel()      # a handle of the wrong kind
    _ffi.debug_path()
    fn = L.skdsp_convcode_encode_rows_dev
    assert fn(ctypes.c_void_p(vit.h), p(), 4, 1, None, 0, p(64), None) == -1 and b"not a convolutional code handle" in L.skdsp_last_error()
    assert fn(ctypes.c_void_p(enc.h), None, 4, 1, None, 0, p(64), None) == -1 and fn(ctypes.c_void_p(enc.h), p(), 4, 1, None, 0, None, None) == -1
    assert fn(ctypes.c_void_p(enc.h), p(), 4, 2, None, 1, p(64), None) == -1      # a state count without states
    assert fn(ctypes.c_void_p(enc.h), p(), 4, 3, p(128), 2, p(64), None) == -1
    assert fn(ctypes.c_void_p(enc.h), p(), -4, 1, None, 0, p(64), None) == -1
    assert fn(ctypes.c_void_p(enc.h), None, 0, 1, None, 0, None, None) == 0 and fn(ctypes.c_void_p(enc.h), None, 4, 0, None, 0, None, None) == 0
    m1, m2 = 0b011, 0b101
    erase = np.array([3.5])
    assert L.skdsp_puncture_rows_dev(p(), 12, 1, 8, m1, 0b001, 3, p(128)) == -1
    assert L.skdsp_puncture_rows_dev(p(4), 12, 1, 8, m1, m2, 3, p(128)) == -1 and b"aligned" in L.skdsp_last_error()
    assert L.skdsp_puncture_rows_dev(None, 12, 1, 8, m1, m2, 3, p(128)) == -1 and L.skdsp_puncture_rows_dev(p(), 12, 1, 5, m1, m2, 3, p(128)) == -1
    assert L.skdsp_depuncture_rows_dev(p(), 8, 1, 8, m1, m2, 3, None, p(128)) == -1 and b"erase" in L.skdsp_last_error()
    assert L.skdsp_depuncture_rows_dev(p(), 8, 1, 8, m1, m2, 3, _ffi._ptr(erase), None) == -1
    assert L.skdsp_puncture_rows_dev(None, 4, 1, 8, m1, m2, 3, None) == 0 and L.skdsp_puncture_rows_dev(None, 12, 0, 8, m1, m2, 3, None) == 0      # no period / no rows
    assert L.skdsp_bit_count_rows_dev(p(), 8, p(64), 8, 8, 1, 0, p(132)) == -1 and b"8-byte" in L.skdsp_last_error()
    assert L.skdsp_bit_count_rows_dev(None, 8, p(64), 8, 8, 1, 0, p(128)) == -1 and L.skdsp_bit_count_rows_dev(p(), 8, p(64), 8, 8, 1, 0, None) == -1
    assert L.skdsp_bit_count_rows_dev(p(), -1, p(64), 8, 8, 1, 0, p(128)) == -1
    assert L.skdsp_bit_count_rows_dev(None, 8, None, 8, 8, 0, 0, None) == 0
    assert _ffi.debug_path() == []
    buf.write(np.full(8, 7, dtype=np.uint8), 128)
    assert L.skdsp_bit_count_rows_dev(None, 0, None, 0, 0, 1, 0, p(128)) == 0 and not buf.read(128, 8).any() and _ffi.debug_path() == []      # n = 0: zero counts, no launch
    buf.free()


# ---------------------------------------------------------------------------------------------------------------- host forms against device forms
@pytest.mark.parametrize("nrow,n", [(1, 1), (3, 67), (2, 300)])
def test_encoder_host_form_equals_the_device_form_with_states_per_row(nrow, n):
    """skdsp_convcode_encode_rows (host pointers: the bits, the per-row initial states, the code and states_out are staged) against
    skdsp_convcode_encode_rows_dev on the same data, bit for bit; also one shared state and no state, with and without states_out"""
    rng = np.random.default_rng(63 + n)
    for G in (('1111001', '1011011'), ('11110111', '11011001', '10010101')):
        k, K, R = _ffi.ConvCodeKernel(G), len(G[0]), len(G)
        bits = rng.integers(0, 2, (nrow, n), dtype=np.uint8)
        dbits, dcode, dst, dso = _ffi.DeviceBytes(bits.size), _ffi.DeviceBytes(R * bits.size), _ffi.DeviceBytes(nrow), _ffi.DeviceBytes(nrow)
        dbits.write(bits.reshape(-1))
        for nst in (nrow, 1, 0):
            st = rng.integers(0, 1 << (K - 1), nst).astype(np.uint8)
            code, out = k.encode_rows(bits, st if nst else None)
            if nst:
                dst.write(st)
            k.encode_rows_dev(dbits.ptr, n, nrow, dst.ptr if nst else 0, nst, dcode.ptr, dso.ptr)
            assert np.array_equal(dcode.read(), code.reshape(-1)) and np.array_equal(dso.read(), out), (G, nst)
            code2 = np.empty_like(code)      # states_out not wanted: the same code bits
            _ffi.check(_ffi.load().skdsp_convcode_encode_rows(ctypes.c_void_p(k.h), _ffi._ptr(bits), n, nrow, _ffi._ptr(st), nst, _ffi._ptr(code2), None))
            assert np.array_equal(code2, code), (G, nst)


@pytest.mark.parametrize("nrow,n", [(1, 1), (3, 131), (2, 700)])
def test_bit_count_host_form_equals_the_device_form(nrow, n):
    """skdsp_bit_count_rows (host pointers, rows at two different strides) against skdsp_bit_count_rows_dev and NumPy"""
    rng = np.random.default_rng(64 + n)
    tx, rx = rng.integers(0, 2, (nrow, n + 5), dtype=np.uint8), rng.integers(0, 2, (nrow, n), dtype=np.uint8)
    dtx, drx, dcnt = _ffi.DeviceBytes(tx.size), _ffi.DeviceBytes(rx.size), _ffi.DeviceBytes(8 * nrow)
    dtx.write(tx.reshape(-1))
    drx.write(rx.reshape(-1))
    for invert in (False, True):
        got = _ffi.bit_count_rows(tx, rx, invert, n)
        _ffi.bit_count_rows_dev(dtx.ptr, n + 5, drx.ptr, n, n, nrow, invert, dcnt.ptr)
        assert np.array_equal(dcnt.read().view(np.int64), got) and np.array_equal(got, np.sum((tx[:, :n] ^ rx) != invert, axis=1))
