"""The FEC chain around the Viterbi decoder on the host (no GPU): fec_conv.FECConv.conv_encoder / puncture / depuncture and
digitalcom.bit_errors_host against every result captured from the real reference (tests/golden/gen_golden_fecchain.py -> g21_fecchain.npz,
g21_conventions.json), the rows forms' length function against the 1-D methods, the argument conventions, and the kernels' plans, staging
and per-item functions walked thread by thread on the CPU (tests/host/convcode_emul.cpp over csrc/convcode_core.hpp), once more under
-fsanitize=address,undefined with unaligned windows.  Everything is bits or element moves: every comparison is array_equal."""
import ctypes
import inspect
import json
import os
import subprocess
import warnings

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, digitalcom as dc, fec_conv as fc
from conftest import GOLDEN, ROOT

PATTERNS = [('110', '101'), ('1101', '1011'), ('1', '1'), ('1001011', '1110100')]
UNEQUAL = ('1000101', '1111010')        # keeps 3 and 5 bits: the reference's puncture fails on it, the rows forms refuse it
LEADING_ZERO = [('0111', '0101'), ('0111', '1101', '1011')]
EDGE_CODES = [('111', '101'), ('1111001', '1011011'), ('111101011', '101110001'), ('11110111', '11011001', '10010101')] + LEADING_ZERO


@pytest.fixture(scope="module")
def g21():
    g = np.load(os.path.join(GOLDEN, "g21_fecchain.npz"))
    return g, {name: json.loads(str(g[name])) for name in ("enc", "punct", "ber")}


@pytest.fixture(scope="module")
def conv21():
    return json.load(open(os.path.join(GOLDEN, "g21_conventions.json")))


def code_of(G, cache={}):
    G = tuple(G)
    if G not in cache:
        cache[G] = fc.FECConv(G, 10)
    return cache[G]


def caught(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = fn()
    return r, [str(v.message) for v in w]


def unequal(pattern):
    return pattern[0].count('1') != pattern[1].count('1') or len(pattern[0]) != len(pattern[1])


def edge_lengths(K, plan):
    return sorted({1, K - 2, K - 1, K, 15, 16, 17, 63, 64, 65, plan["run"] - 1, plan["run"], plan["run"] + 1, plan["wg"] - 1, plan["wg"] + 1})


def random_state(rng, K):
    return "".join(str(v) for v in rng.integers(0, 2, K - 1))


# ---------------------------------------------------------------------------------------------------------------- the captured cases
def test_fixture_covers_what_the_issue_lists(g21):
    g, cases = g21
    assert {(len(c["G"]), len(c["G"][0])) for c in cases["enc"]} >= {(2, 3), (2, 5), (2, 7), (2, 9), (3, 3), (3, 6), (3, 8)}
    assert {tuple(c["G"]) for c in cases["enc"]} >= set(LEADING_ZERO)
    for G in {tuple(c["G"]) for c in cases["enc"]}:
        K = len(G[0])
        assert {c["n"] for c in cases["enc"] if tuple(c["G"]) == G} == {1, K - 2, K - 1, K, 17, 200}
    assert {tuple(c["pattern"]) for c in cases["punct"]} == set(PATTERNS) | {UNEQUAL}
    assert {c["erase_value"] for c in cases["punct"] if c["fn"] == "depuncture"} == {3.5, -2.25}
    seen = {w for c in cases["punct"] for w in c.get("warnings", [])}
    assert seen >= {'Number of code bits must be even!', 'Truncating bits to be compatible.', 'Number of soft bits must be even!',
                    'The number of soft bits is not a multiple', 'Truncating soft bits to be compatible.'}
    assert any(c["fn"] == "puncture" and "raises" in c for c in cases["punct"] if tuple(c["pattern"]) == UNEQUAL)
    assert len(cases["ber"]) >= 30 and {c["n_corr"] for c in cases["ber"]} == {64, 256, 1024} and {c["n_transient"] for c in cases["ber"]} == {0, 7}
    assert {c["kmax"] for c in cases["ber"]} == {0, 1} and min(c["taumax"] for c in cases["ber"]) == -20 and max(c["taumax"] for c in cases["ber"]) == 20
    assert any(c["errors"] == 0 for c in cases["ber"]) and any(c["same"] for c in cases["ber"])
    assert any(g[c["key"] + "_rx"].size > g[c["key"] + "_tx"].size for c in cases["ber"]) and any(g[c["key"] + "_rx"].size < g[c["key"] + "_tx"].size for c in cases["ber"])
    assert any(g[c["key"] + "_tx"].size - c["n_transient"] < c["n_corr"] for c in cases["ber"])


def test_conv_encoder_equals_every_reference_case(g21, conv21):
    g, cases = g21
    for c in cases["enc"]:
        y, s = code_of(c["G"]).conv_encoder(g[c["key"] + "_in"], c["state"])
        assert type(y).__name__ == c["out_type"] == "ndarray" and str(y.dtype) == c["out_dtype"] == "float64", c["key"]
        assert np.array_equal(y, g[c["key"] + "_out"]) and s == c["state_out"] and isinstance(s, str), c["key"]
    assert conv21["return_types"]["conv_encoder"] == ["ndarray", "str"]


def test_puncture_and_depuncture_equal_every_reference_case(g21):
    g, cases = g21
    cc = code_of(('111', '101'))
    for c in cases["punct"]:
        pat = tuple(c["pattern"])
        if unequal(pat):      # the rows forms refuse it; the 1-D host methods make no claim (g21_conventions.json: patterns)
            with pytest.raises(ValueError):
                _ffi.pattern_masks(pat)
            continue
        x = g[c["key"] + "_in"].astype(np.float64)
        if c["fn"] == "puncture":
            y, w = caught(lambda: cc.puncture(x, pat))
        else:
            y, w = caught(lambda: cc.depuncture(x, pat, c["erase_value"]))
        assert w == c["warnings"], c["key"]
        assert str(y.dtype) == c["out_dtype"] and np.array_equal(y, g[c["key"] + "_out"]), c["key"]


def test_bit_errors_host_equals_every_reference_case(g21, conv21):
    g, cases = g21
    for c in cases["ber"]:
        tx, rx = g[c["key"] + "_tx"], g[c["key"] + "_rx"]
        assert dc.bit_errors_search(tx[c["n_transient"]:], rx[c["n_transient"]:], c["n_corr"]) == (c["kmax"], c["taumax"]), c["key"]
        count, errors = dc.bit_errors_host(tx, tx if c["same"] else rx, c["n_corr"], c["n_transient"])
        assert (count, int(errors)) == (c["count"], c["errors"]), c["key"]
        assert [type(count).__name__, type(errors).__name__] == c["types"] == conv21["return_types"]["bit_errors"] == ["int", "int64"]
        count, errors = dc.bit_errors_host(tx.astype(np.float64), rx.astype(np.float64), c["n_corr"], c["n_transient"])      # the reference's input form
        assert (count, int(errors)) == (c["count"], c["errors"])


def test_signatures_match_reference(conv21):
    for name in ("conv_encoder", "puncture", "depuncture"):
        ours = [[p.name, None if p.default is p.empty else (list(p.default) if isinstance(p.default, tuple) else p.default)]
                for p in inspect.signature(getattr(fc.FECConv, name)).parameters.values()]
        assert ours == conv21["signatures"][name], name
    for f in (dc.bit_errors, dc.bit_errors_host):
        assert [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(f).parameters.values()] == conv21["signatures"]["bit_errors"]
    assert inspect.signature(fc.FECConv.puncture_rows).parameters["puncture_pattern"].default == ('110', '101')
    assert inspect.signature(fc.FECConv.depuncture_rows).parameters["erase_value"].default == 3.5


def test_conventions_are_settled_before_any_device_call(conv21):
    assert set(conv21["deliberate_differences"]) == {"bit_values", "odd_n_corr", "n_corr_max", "ties", "empty", "patterns", "rows"}
    ref = conv21["bit_errors"]
    assert "raises" not in ref["value_2"] and ref["odd_n_corr"]["warnings"] == ["n_corr needs to be even"]
    b = np.random.default_rng(21).integers(0, 2, 300)
    for f in (dc.bit_errors, dc.bit_errors_host):
        for bad in (np.where(np.arange(300) == 5, 2, b), np.where(np.arange(300) == 5, -1, b), b + 0.5):                      # deliberate: bit_values
            with pytest.raises(ValueError, match="0 / 1"):
                f(bad, b)
            with pytest.raises(ValueError, match="0 / 1"):
                f(b, bad)
        with pytest.warns(UserWarning, match="n_corr needs to be even"):                                                         # deliberate: odd_n_corr
            with pytest.raises(ValueError, match="even"):
                f(b, b, 255)
        with pytest.raises(ValueError, match="65536"):                                                                           # deliberate: n_corr_max
            f(b, b, 65538)
        with pytest.raises(ValueError, match="transient"):                                                                       # deliberate: empty
            f(b, b, 64, 300)
        with pytest.raises(ValueError):
            f(b.reshape(2, 150), b)
    # deliberate: ties -- two streams whose exact correlation is flat pick phase 0, lag -n_corr / 2 (the first index)
    assert dc.bit_errors_search(np.zeros(64, int), np.zeros(64, int), 64) == (0, -32)
    assert dc.bit_errors_search(np.zeros(64, int), np.ones(64, int), 64) == (1, -32)
    cc = code_of(('111', '101'))
    for bad in (('110', '1011'), ('110', '100'), ('1' * 65, '1' * 65), ('000', '000'), ('110',), ('1a0', '101')):                # deliberate: patterns
        for f in (cc.puncture_rows, cc.depuncture_rows):
            with pytest.raises(ValueError):
                f(np.zeros((2, 12)), bad)
    assert conv21["unequal_patterns"]["puncture_unequal_ones"]["raises"] == "ValueError" and conv21["unequal_patterns"]["puncture_unequal_length"]["raises"] == "IndexError"
    for f in (cc.conv_encoder_rows, cc.puncture_rows, cc.depuncture_rows):
        with pytest.raises(ValueError, match="2-D"):
            f(np.zeros(12))
    with pytest.raises(ValueError, match="0 / 1"):
        cc.conv_encoder_rows(np.full((2, 5), 2))
    for bad in ('0', '012', ['00'], ['00', '0', '00'], [0, 0]):
        with pytest.raises(ValueError):
            cc.conv_encoder_rows(np.zeros((2, 5), int), bad)
    y, s = cc.conv_encoder_rows(np.zeros((3, 0), int), ['00', '01', '10'])                                                    # nothing to encode: no device call
    assert y.shape == (3, 0) and y.dtype == np.float64 and s == ['00', '01', '10']
    with pytest.raises(ValueError, match="0 / 1"):
        dc.bit_errors_rows(np.full((2, 5), 2), np.zeros((2, 5)))


def test_c_abi_rejects_bad_arguments_without_a_device():
    L = _ffi.load()
    h = ctypes.c_void_p(0)

    def create(*polys):
        arr = (ctypes.c_char_p * len(polys))(*[p.encode() for p in polys])
        return L.skdsp_convcode_create(arr, len(polys), ctypes.byref(h))
    assert create('111') == -1 and b"Rate 1/2 or 1/3" in L.skdsp_last_error()
    assert create('111', '10') == -1 and create('11', '10') == -1 and create('1' * 10, '1' * 10) == -1 and create('121', '101') == -1
    assert h.value is None
    assert L.skdsp_convcode_create((ctypes.c_char_p * 2)(b'111', b'101'), 2, None) == -1
    for name in ("encode_rows", "encode_rows_dev"):
        assert getattr(L, "skdsp_convcode_" + name)(None, None, 1, 1, None, 0, None, None) == -1 and b"not a convolutional code handle" in L.skdsp_last_error()
    assert create('111', '101') == 0
    for name in ("encode_rows", "encode_rows_dev"):
        fn = getattr(L, "skdsp_convcode_" + name)
        assert fn(h, None, -1, 1, None, 0, None, None) == -1 and fn(h, None, 1, -1, None, 0, None, None) == -1
        assert fn(h, None, 4, 3, None, 2, None, None) == -1 and b"initial states" in L.skdsp_last_error()      # 2 states for 3 rows
        assert fn(h, None, 4, 1, None, 0, None, None) == -1 and b"null pointer" in L.skdsp_last_error()
        assert fn(h, None, 4, 0, None, 0, None, None) == 0 and fn(h, None, 0, 3, None, 0, None, None) == 0     # no rows / no bits and no state wanted: no-ops
    st = np.array([4], dtype=np.uint8)
    assert L.skdsp_convcode_encode_rows(h, _ffi._ptr(st), 1, 1, _ffi._ptr(st), 1, _ffi._ptr(st), None) == -1 and b"does not fit" in L.skdsp_last_error()
    out = np.full(3, 9, dtype=np.uint8)
    assert L.skdsp_convcode_encode_rows(h, None, 0, 3, _ffi._ptr(np.array([2], np.uint8)), 1, None, _ffi._ptr(out)) == 0 and out.tolist() == [2, 2, 2]
    L.skdsp_destroy(h)
    n_out = ctypes.c_int64(-1)
    m = lambda p: int(p[::-1], 2)      # noqa: E731
    for fn in (L.skdsp_puncture_out_len, L.skdsp_depuncture_out_len):
        assert fn(10, m('110'), m('101'), 3, None) == -1
        assert fn(-1, m('110'), m('101'), 3, ctypes.byref(n_out)) == -1
        assert fn(10, m('110'), m('100'), 3, ctypes.byref(n_out)) == -1 and b"same number" in L.skdsp_last_error()
        assert fn(10, m('110'), m('101'), 65, ctypes.byref(n_out)) == -1 and fn(10, m('110'), m('101'), 0, ctypes.byref(n_out)) == -1
        assert fn(10, m('1101'), m('101'), 3, ctypes.byref(n_out)) == -1 and b"beyond" in L.skdsp_last_error()
        assert fn(10, 0, 0, 3, ctypes.byref(n_out)) == -1
    assert L.skdsp_puncture_out_len(61, m('110'), m('101'), 3, ctypes.byref(n_out)) == 0 and n_out.value == 40
    erase = np.array([3.5])
    for fn, extra in ((L.skdsp_puncture_rows, ()), (L.skdsp_puncture_rows_dev, ()), (L.skdsp_depuncture_rows, (_ffi._ptr(erase),)), (L.skdsp_depuncture_rows_dev, (_ffi._ptr(erase),))):
        assert fn(None, 12, 1, 3, m('110'), m('101'), 3, *extra, None) == -1 and b"1, 2, 4 or 8" in L.skdsp_last_error()
        assert fn(None, 12, 1, 8, m('110'), m('100'), 3, *extra, None) == -1
        assert fn(None, 12, 1, 8, m('110'), m('101'), 3, *extra, None) == -1 and b"null pointer" in L.skdsp_last_error()
        assert fn(None, 2 ** 31, 1, 8, m('110'), m('101'), 3, *extra, None) == -1
        assert fn(None, 12, 0, 8, m('110'), m('101'), 3, *extra, None) == 0 and fn(None, 2, 5, 8, m('110'), m('101'), 3, *extra, None) == 0     # no rows / no period
    for fn in (L.skdsp_depuncture_rows, L.skdsp_depuncture_rows_dev):
        assert fn(None, 12, 1, 8, m('110'), m('101'), 3, None, None) == -1 and b"erase" in L.skdsp_last_error()
    for fn in (L.skdsp_bit_count_rows, L.skdsp_bit_count_rows_dev):
        assert fn(None, 8, None, 8, -1, 1, 0, None) == -1 and fn(None, -8, None, 8, 4, 1, 0, None) == -1 and fn(None, 8, None, 8, 4, -1, 0, None) == -1
        assert fn(None, 8, None, 8, 4, 1, 0, None) == -1
        assert fn(None, 8, None, 8, 4, 0, 0, None) == 0
    counts = np.full(2, 7, dtype=np.int64)
    assert L.skdsp_bit_count_rows(None, 0, None, 0, 0, 2, 0, _ffi._ptr(counts)) == 0 and counts.tolist() == [0, 0]
    assert L.skdsp_bit_count_rows(None, 8, None, 8, 4, 1, 0, _ffi._ptr(counts)) == -1 and b"null pointer" in L.skdsp_last_error()
    assert _ffi.debug_path() == []


def test_rows_length_function_equals_the_1d_methods():
    cc = code_of(('111', '101'))
    for pat in PATTERNS:
        for n in range(0, 75):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert _ffi.puncture_out_len(n, pat) == len(cc.puncture(np.zeros(n), pat)), (pat, n)
                assert _ffi.puncture_out_len(n, pat, True) == len(cc.depuncture(np.zeros(n), pat)), (pat, n)


# ---------------------------------------------------------------------------------------------------------------- the kernels' plan on the CPU
def build_emul(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "convcode_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("cvc"), "convcode_emul", [])


def plan_of(exe):
    """{run, wg, cnt_wg, gather_item, threads} of the kernels' work split"""
    words = subprocess.check_output([exe, "plan"]).decode().split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def emul_enc(exe, tmp, G, bits2d, states, in_off=0, out_off=0):
    """(code (nrow, R n) uint8, final state numbers) through the emulation; states: list of strings (0, 1 or nrow of them)"""
    bits2d = np.asarray(bits2d, dtype=np.uint8)
    f = [str(tmp / name) for name in ("st_in.u8", "in.u8", "out.u8", "st_out.u8")]
    np.array([int(s, 2) for s in states], dtype=np.uint8).tofile(f[0])
    bits2d.tofile(f[1])
    subprocess.check_call([exe, "enc", ",".join(G), str(bits2d.shape[1]), str(bits2d.shape[0]), str(len(states))] + f + [str(in_off), str(out_off)])
    return np.fromfile(f[2], dtype=np.uint8).reshape(bits2d.shape[0], -1), np.fromfile(f[3], dtype=np.uint8)


def emul_gather(exe, tmp, dep, x2d, pat, erase=None, in_off=0, out_off=0):
    x2d = np.ascontiguousarray(x2d)
    fin, fout = str(tmp / "g_in.bin"), str(tmp / "g_out.bin")
    x2d.tofile(fin)
    e = 0 if erase is None else int(np.array([erase]).astype(x2d.dtype).view("u%d" % x2d.dtype.itemsize)[0])
    subprocess.check_call([exe, "gat", str(int(dep)), str(x2d.shape[1]), str(x2d.shape[0]), str(x2d.dtype.itemsize), pat[0], pat[1], "%x" % e, fin, fout,
                           str(in_off), str(out_off)])
    return np.fromfile(fout, dtype=x2d.dtype).reshape(x2d.shape[0], -1)


def emul_count(exe, tmp, tx2d, rx2d, n, invert, tx_off=0, rx_off=0):
    tx2d, rx2d = np.ascontiguousarray(tx2d, dtype=np.uint8), np.ascontiguousarray(rx2d, dtype=np.uint8)
    ft, fr = str(tmp / "c_tx.u8"), str(tmp / "c_rx.u8")
    nrow = tx2d.shape[0]
    tx2d.reshape(-1)[:(nrow - 1) * tx2d.shape[1] + n].tofile(ft)
    rx2d.reshape(-1)[:(nrow - 1) * rx2d.shape[1] + n].tofile(fr)
    out = subprocess.check_output([exe, "cnt", str(n), str(nrow), str(tx2d.shape[1]), str(rx2d.shape[1]), str(int(invert)), ft, fr, str(tx_off), str(rx_off)])
    return np.array([int(v) for v in out.split()], dtype=np.int64)


def host_rows(cc, bits2d, states):
    """conv_encoder of every row: (code (nrow, R n) float64, [state strings])"""
    rows = [cc.conv_encoder(bits2d[r], states[r if len(states) > 1 else 0]) for r in range(bits2d.shape[0])]
    return np.array([r[0] for r in rows]).reshape(bits2d.shape[0], -1), [r[1] for r in rows]


def host_gather_rows(cc, dep, x2d, pat, erase=3.5):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows = [cc.depuncture(x, pat, erase) if dep else cc.puncture(x, pat) for x in x2d]
    return np.array(rows).reshape(x2d.shape[0], -1)


def gather_row_lengths(pat, dep):
    """elements per input row: 0 periods, 1 period, odd, a non-multiple, and output rows ending 1 byte either side of a 16-byte boundary"""
    per_in = 2 * pat[0].count('1') if dep else 2 * len(pat[0])
    per_out = 2 * len(pat[0]) if dep else 2 * pat[0].count('1')
    lens = {max(per_in - 2, 0), per_in, per_in + 1, 3 * per_in + 2, 5 * per_in + 1}
    for periods in range(1, 40):      # (uint8 elements: an output row of 16 m +- 1 bytes where the period allows it)
        if (periods * per_out) % 16 in (1, 15):
            lens.add(periods * per_in)
    return sorted(lens)


def test_plan_is_what_the_kernels_document(emul):
    p = plan_of(emul)
    assert p == {"run": 16, "wg": 4096, "cnt_wg": 4096, "gather_item": 1024, "threads": 256} and p["wg"] == p["run"] * p["threads"]
    assert subprocess.check_output([emul, "len", "0", "61", "110", "101"]).split() == [b"40"]
    assert subprocess.call([emul, "len", "0", "61", "110", "100"]) == 5


def test_emulated_encoder_equals_the_fixtures_and_the_host_method(g21, emul, tmp_path):
    g, cases = g21
    for c in cases["enc"]:
        y, s = emul_enc(emul, tmp_path, c["G"], g[c["key"] + "_in"][None], [c["state"]])
        assert np.array_equal(y[0], g[c["key"] + "_out"]) and fc.binary(int(s[0]), len(c["state"])) == c["state_out"], c["key"]
    plan = plan_of(emul)
    rng = np.random.default_rng(211)
    for G in EDGE_CODES:
        cc, K = code_of(G), len(G[0])
        for i, n in enumerate(edge_lengths(K, plan)):
            for state in ('1' * (K - 1), random_state(rng, K)):
                bits = rng.integers(0, 2, (1, n))
                off = (0, 1, 3, 15)[i % 4]
                y, s = emul_enc(emul, tmp_path, G, bits, [state], off, (0, 1, 3, 15)[(i + 1) % 4])
                ref, sref = host_rows(cc, bits, [state])
                assert np.array_equal(y, ref) and [fc.binary(int(v), K - 1) for v in s] == sref, (G, n, state, off)
    for G in (('1111001', '1011011'), ('11110111', '11011001', '10010101')):      # rows: n odd, one state per row / one for all / rest
        cc, K = code_of(G), len(G[0])
        bits = rng.integers(0, 2, (3, 4099))
        for states in ([random_state(rng, K) for _ in range(3)], [random_state(rng, K)], []):
            y, s = emul_enc(emul, tmp_path, G, bits, states, 3, 1)
            ref, sref = host_rows(cc, bits, states or ['0' * (K - 1)])
            assert np.array_equal(y, ref) and [fc.binary(int(v), K - 1) for v in s] == sref, (G, len(states))


def test_emulated_gathers_equal_the_host_methods(emul, tmp_path):
    cc = code_of(('111', '101'))
    rng = np.random.default_rng(212)
    plan = plan_of(emul)
    for pat in PATTERNS:
        for dep in (False, True):
            lens = gather_row_lengths(pat, dep) + [plan["gather_item"] * 3 + 7]      # (more than one item per row)
            for i, n in enumerate(lens):
                x = rng.integers(0, 2, (3, n)).astype(np.uint8)
                off = (0, 1, 3, 15)[i % 4]
                y = emul_gather(emul, tmp_path, dep, x, pat, 7 if dep else None, off, (0, 1, 3, 15)[(i + 2) % 4])
                assert np.array_equal(y, host_gather_rows(cc, dep, x, pat, 7)), (pat, dep, n)
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        x = rng.integers(0, 60, (2, 67)).astype(dt)
        for pat in PATTERNS:
            assert np.array_equal(emul_gather(emul, tmp_path, False, x, pat, None, 1, 3), host_gather_rows(cc, False, x, pat)), (dt, pat)
            y = emul_gather(emul, tmp_path, True, x, pat, 3.5, 3, 1)
            assert np.array_equal(y, host_gather_rows(cc, True, x.astype(np.float64), pat, float(np.array([3.5]).astype(dt)[0]))), (dt, pat)
    y = emul_gather(emul, tmp_path, True, np.zeros((1, 8), np.int16), ('110', '101'), 3.5)[0]                               # int16: 3.5 -> 3
    assert y.tolist() == [0, 0, 0, 3, 3, 0] * 2


def test_emulated_count_equals_numpy(emul, tmp_path):
    rng = np.random.default_rng(213)
    for n in (1, 15, 16, 17, 4095, 4097, 65539):
        for nrow in (1, 5):
            tx, rx = rng.integers(0, 2, (nrow, n + 9)), rng.integers(0, 2, (nrow, n + 2))
            for invert in (0, 1):
                got = emul_count(emul, tmp_path, tx, rx, n, invert, (0, 1, 3, 15)[n % 4], (15, 3, 1, 0)[n % 4])
                assert np.array_equal(got, np.sum((tx[:, :n] ^ rx[:, :n]) ^ invert, axis=1)), (n, nrow, invert)


def test_sanitized_emulation_at_unaligned_windows(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation: every kernel, several work items with a partial last one, the windows 0, 1, 3
    and 15 bytes off a 16-byte boundary inside exact-size allocations (a staging overrun shows here, not on a GPU)"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "convcode_emul_san", san)
    plan = plan_of(exe)
    rng = np.random.default_rng(214)
    cc2 = code_of(('111', '101'))
    for G in (('111', '101'), ('111101011', '101110001'), ('11110111', '11011001', '10010101'), ('0111', '1101', '1011')):
        cc, K = code_of(G), len(G[0])
        for n in (1, K - 2, K - 1, plan["run"] + 1, plan["wg"] - 1, 2 * plan["wg"] + 5):
            bits = rng.integers(0, 2, (2, n))
            states = [random_state(rng, K), random_state(rng, K)]
            ref, sref = host_rows(cc, bits, states)
            for in_off, out_off in ((0, 0), (1, 3), (3, 15), (15, 1)):
                y, s = emul_enc(exe, tmp_path, G, bits, states, in_off, out_off)
                assert np.array_equal(y, ref) and [fc.binary(int(v), K - 1) for v in s] == sref, (G, n, in_off, out_off)
    for pat in PATTERNS:
        for dep in (False, True):
            for n in (gather_row_lengths(pat, dep)[1], 2 * plan["gather_item"] + 11):
                x = rng.integers(0, 2, (3, n)).astype(np.uint8)
                for in_off, out_off in ((0, 0), (1, 3), (3, 15), (15, 1)):
                    assert np.array_equal(emul_gather(exe, tmp_path, dep, x, pat, 9, in_off, out_off), host_gather_rows(cc2, dep, x, pat, 9)), (pat, dep, n)
            x = rng.integers(-9, 9, (2, 131)).astype(np.float64)
            assert np.array_equal(emul_gather(exe, tmp_path, dep, x, pat, 3.5, 1, 3), host_gather_rows(cc2, dep, x, pat, 3.5))
    for n in (1, 17, plan["cnt_wg"] + 3):
        tx, rx = rng.integers(0, 2, (3, n + 4)), rng.integers(0, 2, (3, n))
        for t_off, r_off in ((0, 0), (1, 3), (3, 15), (15, 1)):
            assert np.array_equal(emul_count(exe, tmp_path, tx, rx, n, 1, t_off, r_off), np.sum((tx[:, :n] ^ rx) ^ 1, axis=1))
