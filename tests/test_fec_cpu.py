"""fec_conv.FECConv on the host (no GPU): the float64 restatement of the Viterbi decoder, the encoder and the puncturing helpers
against results captured from the real reference (tests/golden/gen_golden_fec.py -> g19_fec.npz, g19_conventions.json), the argument
conventions, and the kernel's per-state step walked lane by lane on the CPU (tests/host/viterbi_emul.cpp over csrc/viterbi_core.hpp)."""
import inspect
import json
import os
import subprocess
import warnings

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, fec_conv as fc
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def g19():
    g = np.load(os.path.join(GOLDEN, "g19_fec.npz"))
    return g, json.loads(str(g["cases"])), json.loads(str(g["host"]))


@pytest.fixture(scope="module")
def conv():
    return json.load(open(os.path.join(GOLDEN, "g19_conventions.json")))


def received(x):
    """a stored array as the reference was handed it"""
    return x.astype(np.int64) if x.dtype.kind == "i" else x.astype(np.float64)


def test_fixture_covers_what_the_decoder_must_do(g19):
    g, cases, host = g19
    groups = {c["group"] for c in cases}
    assert groups == {"codes", "metrics", "depths", "ties", "carry", "lengths"}
    assert {(len(c["G"]), len(c["G"][0])) for c in cases if c["group"] == "codes"} == {(2, k) for k in range(3, 10)} | {(3, k) for k in range(3, 9)}
    assert {c["depth"] for c in cases if c["group"] == "depths"} == {1, 2, 10, 31, 32, 33, 63, 64, 65, 100, 128}
    assert any(c["calls"] == 3 and len(g[c["key"] + "_y1"]) == 0 for c in cases)       # a call too short to emit, state still advances
    for c in cases:
        if c["group"] == "codes":   # the error pattern is pinned, not only the message
            assert int(c["note"].split()[0]) > 0, c


def test_host_restatement_equals_every_reference_case(g19):
    g, cases, _ = g19
    for c in cases:
        cc = fc.FECConv(tuple(c["G"]), c["depth"])
        for i in range(c["calls"]):
            y = cc.viterbi_decoder_host(received(g["%s_x%d" % (c["key"], i)]), c["metric"], c["quant_level"])
            ref = g["%s_y%d" % (c["key"], i)]
            assert y.dtype == np.float64 and y.shape == ref.shape, (c["key"], i, y.shape, ref.shape)
            assert np.array_equal(y, ref), (c["key"], i, int(np.sum(y != ref)))


def test_host_state_carry_reset_and_from_rest(g19):
    g, cases, _ = g19
    c = next(c for c in cases if c["key"] == "carry_soft_h7")
    xs = [received(g["carry_soft_h7_x%d" % i]) for i in range(3)]
    cc = fc.FECConv(tuple(c["G"]), c["depth"])
    first = cc.viterbi_decoder_host(xs[0])
    again = cc.viterbi_decoder_host(xs[0])
    assert first.shape == again.shape and not np.array_equal(first, again)       # the second call continues the first
    assert np.array_equal(cc.viterbi_decoder_host(xs[0], carry=False), first)    # from rest, state untouched ...
    cc2 = fc.FECConv(tuple(c["G"]), c["depth"])
    cc2.viterbi_decoder_host(xs[0])
    cc2.viterbi_decoder_host(xs[0])
    assert np.array_equal(cc.viterbi_decoder_host(xs[2]), cc2.viterbi_decoder_host(xs[2]))   # ... so both objects are two calls in
    cc.reset()
    assert np.array_equal(cc.viterbi_decoder_host(xs[0]), first)


def test_rows_restatement_is_the_row_by_row_restatement():
    rng = np.random.default_rng(11)
    for G, D, metric, n in ((('111', '101'), 10, 'soft', 120), (('11111', '11011', '10101'), 70, 'unquant', 240), (('11111001', '10100111'), 33, 'hard', 151)):
        cc = fc.FECConv(G, D)
        x = rng.integers(0, 2, (5, n)) if metric == 'hard' else rng.uniform(-1, 8, (5, n)) / (7 if metric == 'unquant' else 1)
        y = cc.viterbi_decoder_rows_host(x, metric)
        assert y.shape == (5, -(-n // len(G)) - D + 1) and y.dtype == np.float64
        for r in range(5):
            assert np.array_equal(y[r], cc.viterbi_decoder_host(x[r], metric, carry=False)), (G, r)


def test_encoder_and_puncturing_equal_the_reference(g19):
    g, _, host = g19
    assert {h["fn"] for h in host} == {"conv_encoder", "puncture", "depuncture"}
    seen_warnings = set()
    for h in host:
        x, ref = g[h["key"] + "_in"], g[h["key"] + "_out"]
        if h["fn"] == "conv_encoder":
            cc = fc.FECConv(tuple(h["G"]), 10)
            y, s = cc.conv_encoder(x.astype(np.int64), h["state"])
            assert s == h["state_out"] and isinstance(s, str), h
        else:
            cc = fc.FECConv(('111', '101'), 10)
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                if "erase_value" in h:
                    y = cc.depuncture(x, tuple(h["pattern"]), h["erase_value"])
                else:
                    y = getattr(cc, h["fn"])(x, tuple(h["pattern"]))
            assert [str(v.message) for v in w] == h["warnings"], h
            seen_warnings.update(h["warnings"])
        assert str(y.dtype) == h["out_dtype"] and np.array_equal(y, ref), h
    assert len(seen_warnings) == 7   # every truncation warning of both helpers was triggered


def test_encoder_matches_the_trellis_tables():
    """the decoder's branch words are the encoder's outputs: one step from every state under both inputs"""
    for G in (('111', '101'), ('1111001', '1011011'), ('11110111', '11011001', '10010101'), ('011', '101'), ('011', '110', '101')):
        cc = fc.FECConv(G, 5)
        K, R = len(G[0]), len(G)
        for m in range(cc.Nstates):
            u = m >> (K - 2)
            for p, word in ((cc._p0[m], cc._bits1[m]), (cc._p1[m], cc._bits2[m])):
                out, s = cc.conv_encoder([u], fc.binary(int(p), K - 1))
                assert int(s, 2) == m
                assert int("".join(str(int(v)) for v in out), 2) == word, (G, m, p)


def test_signatures_match_reference(conv):
    for name, sig in conv["signatures"].items():
        ours = [[p.name, None if p.default is p.empty else (list(p.default) if isinstance(p.default, tuple) else p.default)]
                for p in inspect.signature(getattr(fc.FECConv, name)).parameters.values()]
        assert ours == sig, name
    assert list(inspect.signature(fc.FECConv.viterbi_decoder_rows).parameters)[2:] == list(inspect.signature(fc.FECConv.viterbi_decoder).parameters)[2:]


def test_conventions_are_settled_before_any_device_call(conv, caplog):
    """what the reference raises, this raises with the same type (host restatement and GPU entry share the checks); the deliberate
    differences are the ones the fixture names"""
    assert set(conv["deliberate_differences"]) == {"cumulative_metric", "non_finite", "x_2d", "soft_range", "metric_family", "containers",
                                                   "encoder_input", "plots"}
    rng = np.random.default_rng(5)
    xs = np.round(rng.uniform(0, 7, 60) * 4) / 4
    xb = rng.integers(0, 2, 60)
    with caplog.at_level("INFO"):
        cc = fc.FECConv(('111', '101'), 10)
        fc.FECConv(('111', '111', '101'), 10)
    assert [r.getMessage() for r in caplog.records] == ["Rate 1/2 Object", "Rate 1/3 Object"]
    assert not hasattr(cc, "paths")

    def raises(key, fn, entry=None):
        entry = conv[key] if entry is None else entry
        exc = {"ValueError": ValueError, "IndexError": IndexError, "OverflowError": ValueError}[entry["raises"]]
        for f in (cc.viterbi_decoder, cc.viterbi_decoder_host):
            with pytest.raises(exc):
                fn(f)
    for key in ("one_poly", "four_polys"):
        with pytest.warns(UserWarning, match="Invalid rate"), pytest.raises(ValueError, match=conv[key]["message"]):
            fc.FECConv(('111',) if key == "one_poly" else ('111', '101', '110', '011'), 10)
    with pytest.warns(UserWarning, match="Invalid metric type"):
        raises("bad_metric", lambda f: f(xs, 'euclid'))
    raises("hard_float", lambda f: f(xb.astype(np.float64), 'hard'))
    raises("hard_value_2", lambda f: f(np.where(np.arange(60) == 5, 2, xb), 'hard'))
    raises("hard_negative", lambda f: f(np.where(np.arange(60) == 5, -1, xb), 'hard'))
    for bad in (np.nan, np.inf, -np.inf):
        xn = xs.copy()
        xn[7] = bad
        raises("soft_nan" if np.isnan(bad) else "soft_inf", lambda f: f(xn))
        with pytest.raises(ValueError):          # deliberate: the reference mis-compares
            cc.viterbi_decoder(xn, 'unquant')
    raises("soft_odd_count", lambda f: f(xs[:59]))
    raises("unquant_odd_count", lambda f: f(xs[:59], 'unquant'))
    raises("fewer_values_than_depth", lambda f: f(xs[:8]))
    for m in ("soft", "unquant", "hard"):
        raises(None, lambda f: f(np.zeros(0, np.int64 if m == "hard" else np.float64), m), conv["decoder"]["empty"][m])
        with pytest.raises(ValueError, match="viterbi_decoder_rows"):
            cc.viterbi_decoder((xb if m == "hard" else xs).reshape(2, 30), m)
    # what the reference decodes, the restatement decodes to the same shape and dtype
    for name, x in (("list", list(xs)), ("tuple", tuple(xs)), ("float32", xs.astype(np.float32)), ("int64", xs.astype(np.int64))):
        for m in ("soft", "unquant"):
            y = cc.viterbi_decoder_host(x, m, carry=False)
            assert list(y.shape) == conv["decoder"][name][m]["shape"] and str(y.dtype) == conv["decoder"][name][m]["dtype"]
    y = cc.viterbi_decoder_host(xb[:59], 'hard', carry=False)
    assert list(y.shape) == conv["hard_odd_count"]["shape"]
    # the deliberate limits
    for bad in (lambda: cc.viterbi_decoder(np.where(np.arange(60) == 3, 4096.0, xs)), lambda: cc.viterbi_decoder(xs, 'soft', 13),
                lambda: cc.viterbi_decoder(xs, 'soft', -1), lambda: fc.FECConv(('111', '101'), 129), lambda: fc.FECConv(('111', '101'), 0),
                lambda: fc.FECConv(('1111010111', '1011100011'), 10), lambda: fc.FECConv(('11', '10'), 10),
                lambda: cc.conv_encoder([0, 2, 1], '00'), lambda: cc.conv_encoder([0, 1], '000')):
        with pytest.raises(ValueError):
            bad()
    y, s = cc.conv_encoder([], '10')
    assert y.dtype == np.float64 and y.size == 0 and s == '10'
    assert conv["ref_bits_per_s"].keys() == {str(k) for k in range(3, 10)}


def test_c_abi_rejects_bad_arguments_without_a_device():
    import ctypes
    L = _ffi.load()
    h = ctypes.c_void_p(0)

    def create(polys, depth):
        arr = (ctypes.c_char_p * len(polys))(*[p.encode() for p in polys])
        return L.skdsp_viterbi_create(arr, len(polys), depth, ctypes.byref(h))
    assert create(('111', '101'), 129) == -1 and b"128" in L.skdsp_last_error()
    assert create(('111', '101'), 0) == -1
    assert create(('1111010111', '1011100011'), 10) == -1 and b"3 ... 9" in L.skdsp_last_error()
    assert create(('111',), 10) == -1 and create(('111', '10'), 10) == -1 and create(('111', '1x1'), 10) == -1
    assert h.value is None
    assert L.skdsp_viterbi_reset(None) == -1 and L.skdsp_viterbi_decode(None, None, 10, 1, 1, 3, None) == -1


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vit") / "viterbi_emul")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "viterbi_emul.cpp"), "-o", exe])
    return exe


def test_kernel_step_host_emulation_reproduces_the_fixtures(g19, emul, tmp_path):
    """the kernel's own step, trellis and lane mapping, for the one-state-per-lane layouts (K = 3: stream 5 of 16 in the wave; K = 7) and
    the states-per-lane layouts (K = 8: two, K = 9: four), all three metrics, both history widths, and the carried state"""
    g, cases, _ = g19
    want = {"code_h3": 5, "code_t5": 3, "code_h7": 0, "code_t7": 0, "code_h8": 0, "code_t8": 0, "code_h9": 0, "met_hard_t7": 0, "met_unq_gauss_h7": 0,
            "met_unq_gauss_t5": 1, "met_depunct_h7": 0, "depth_h7_1": 0, "depth_h7_64": 0, "depth_h7_65": 0, "depth_h3_128": 15, "tie_zero_h7": 0,
            "tie_alt_h3": 0, "carry_soft_h9": 0, "carry_unq_h7": 0, "carry_hard_h7": 0, "carry_soft_t5": 2, "len_hard_ragged_t5_101": 0,
            "len_hard_ragged_h7_141": 0}
    code = {"hard": 0, "soft": 1, "unquant": 2}
    for c in cases:
        if c["key"] not in want:
            continue
        ins = []
        for i in range(c["calls"]):
            path = str(tmp_path / ("%s_%d.f64" % (c["key"], i)))
            g["%s_x%d" % (c["key"], i)].astype(np.float64).tofile(path)
            ins.append(path)
        outp = str(tmp_path / (c["key"] + ".u8"))
        subprocess.check_call([emul, ",".join(c["G"]), str(c["depth"]), str(code[c["metric"]]), str(c["quant_level"]), str(want[c["key"]]), outp] + ins)
        ref = np.concatenate([g["%s_y%d" % (c["key"], i)] for i in range(c["calls"])])
        assert np.array_equal(np.fromfile(outp, dtype=np.uint8), ref), c["key"]
        want.pop(c["key"])
    assert not want, want
