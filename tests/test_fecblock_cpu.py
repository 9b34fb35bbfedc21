"""fec_block.FECHamming / FECCyclic on the host (no GPU): the vectorised table-form restatement (*_host) against every result captured
from the real reference (tests/golden/gen_golden_fecblock.py -> g20_fecblock.npz, g20_conventions.json), the tables' properties, the
argument conventions, and the kernels' plan, run staging and per-block functions walked thread by thread on the CPU
(tests/host/blockcode_emul.cpp over csrc/blockcode_core.hpp), once more under -fsanitize=address,undefined with unaligned windows."""
import collections
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, fec_block as fb
from conftest import GOLDEN, ROOT

FORM_LANE, FORM_WAVE, FORM_GROUP = 0, 1, 2
NONPRIMITIVE = ('1001', '11111', '100001', '1110101')


@pytest.fixture(scope="module")
def g20():
    g = np.load(os.path.join(GOLDEN, "g20_fecblock.npz"))
    return g, json.loads(str(g["cases"]))


@pytest.fixture(scope="module")
def conv():
    return json.load(open(os.path.join(GOLDEN, "g20_conventions.json")))


def code_of(c, cache={}):
    key = (c["kind"], c["j"], c["G"])
    if key not in cache:
        cache[key] = fb.FECHamming(c["j"]) if c["kind"] == "hamming" else fb.FECCyclic(c["G"])
    return cache[key]


def bits_of(g, c):
    """(what the reference was given, what it returned) for a stored case"""
    x = np.unpackbits(g[c["key"] + "_in"])[:c["nin"]].astype(c["in_dtype"])
    return x, np.unpackbits(g[c["key"] + "_out"])[:c["nout"]].astype(c["out_dtype"])


def method(code, fn, host):
    name = ("hamm_" if isinstance(code, fb.FECHamming) else "cyclic_") + fn + "r" + ("_host" if host else "")
    return getattr(code, name)


def one_error_words(code, rng, nblocks):
    """nblocks code words, every second one with one flipped bit, and a few random words (as int64 bits)"""
    x = rng.integers(0, 2, nblocks * code.k)
    c = method(code, "encode", True)(x).astype(np.int64).reshape(nblocks, code.n)
    rows = np.arange(0, nblocks, 2)
    c[rows, rng.integers(0, code.n, rows.size)] ^= 1
    c[::5] = rng.integers(0, 2, c[::5].shape)
    return x, c.reshape(-1)


def test_fixture_covers_what_the_issue_lists(g20):
    g, cases = g20
    assert {c["j"] for c in cases if c["kind"] == "hamming"} == {3, 4, 5, 6, 7, 8, 10}
    assert {c["G"] for c in cases if c["kind"] == "cyclic"} == {'1011', '10011', '101001', '1100001', '10100001', '101110001', '1101'} | set(NONPRIMITIVE)
    for key in {c["key"].rsplit("_", 1)[0] if c["fn"] == "encode" else None for c in cases} - {None}:
        assert {c["group"] for c in cases if c["key"].startswith(key + "_")} == {"encode", "clean", "one_error", "two_errors", "three_errors", "random"}
    for c in cases:
        n = 2 ** c["j"] - 1
        if c["group"] == "one_error":      # every position for n <= 63, 25 beyond (5 named + 20 random, which may coincide)
            assert c["nin"] == n * n if n <= 63 else 20 * n <= c["nin"] <= 25 * n, c
    assert next(c for c in cases if c["key"] == "ham10_enc")["nout"] == 4 * 1023


def test_host_restatement_equals_every_reference_case(g20):
    g, cases = g20
    for c in cases:
        x, ref = bits_of(g, c)
        y = method(code_of(c), c["fn"], True)(x)
        assert y.dtype == ref.dtype and str(y.dtype) == c["out_dtype"], c["key"]
        assert np.array_equal(y, ref), (c["key"], int(np.sum(y != ref)))
    assert {c["out_dtype"] for c in cases if c["kind"] == "hamming" and c["fn"] == "encode"} == {"float64"}
    assert {c["out_dtype"] for c in cases if not (c["kind"] == "hamming" and c["fn"] == "encode")} == {"int64"}


def test_every_position_has_exactly_one_trap_word(g20):
    _, cases = g20
    for j in range(3, 13):      # Hamming: the syndrome that flips position i is the one s with col[s - 1] - 1 == i; no two positions share one
        enc, syn, trap = fb.hamming_tables(j)
        n, k = 2 ** j - 1, 2 ** j - 1 - j
        col = fb.hamming_columns(j)
        assert enc.dtype == syn.dtype == trap.dtype == np.uint32 and (enc.size, syn.size, trap.size) == (k, n, k)
        assert np.array_equal(enc, col[:k]) and np.array_equal(syn, col) and sorted(col) == list(range(1, n + 1))
        assert trap.min() >= 1 and trap.max() <= n and np.unique(trap).size == k
        assert np.array_equal(col[trap.astype(np.int64) - 1] - 1, np.arange(k))
    for G in sorted({c["G"] for c in cases if c["G"]}):
        # cyclic: run the reference's "switch B" register from EVERY content s and note which outputs it flips (digits of G as the
        # reference reads them); each position must be flipped by exactly one content, and that is trap[i]
        enc, syn, trap = fb.cyclic_tables(G)
        j = len(G) - 1
        k = 2 ** j - 1 - j
        taps = [m for m in range(1, j + 1) if G[m] == '1']
        hits = [[] for _ in range(k)]
        for s in range(2 ** j):
            S = [0] + [(s >> (j - m)) & 1 for m in range(1, j + 1)]
            for i in range(k):
                fbk = sum(S[m] for m in taps) % 2
                S = [0, fbk] + S[1:j]
                if S[1] == 1 and not any(S[2:]):
                    hits[i].append(s)
        assert all(len(h) == 1 for h in hits), G
        assert np.array_equal(trap, [h[0] for h in hits]), G
        assert max(enc.max(), syn.max(), trap.max()) < 2 ** j and trap.min() >= 1


def test_multi_position_syndromes_of_the_non_primitive_codes():
    """one syndrome may flip several positions: a 'syndrome -> one position' table would be wrong for these codes"""
    most = {}
    for G in NONPRIMITIVE + ('10100001',):
        enc, syn, trap = fb.cyclic_tables(G)
        most[G] = max(collections.Counter(trap.tolist()).values())
        s = collections.Counter(trap.tolist()).most_common(1)[0][0]
        c = np.zeros(syn.size, dtype=np.int64)
        c[int(np.flatnonzero(syn == s)[0])] = 1           # one error whose syndrome is s ...
        out = fb.FECCyclic(G).cyclic_decoder_host(c)
        flipped = np.flatnonzero(out != c[:trap.size])
        assert np.array_equal(flipped, np.flatnonzero(trap == s)) and flipped.size == most[G]   # ... flips every position trapped by s
    assert all(v >= 2 for v in most.values()) and most['10100001'] == 2, most
    for G in ('1011', '10011', '101001', '1100001', '1101'):
        assert np.unique(fb.cyclic_tables(G)[2]).size == 2 ** (len(G) - 1) - len(G)


def test_hamming_matrices_equal_the_reference_construction(conv):
    h = fb.FECHamming(3)
    G, H, R, n, k = h.hamm_gen(3)
    assert [type(v).__name__ for v in (G, H, R, n, k)] == conv["hamm_gen"]["types"]
    assert [str(v.dtype) for v in (G, H, R)] == conv["hamm_gen"]["dtypes"] and [list(v.shape) for v in (G, H, R)] == conv["hamm_gen"]["shapes"]
    for j in (3, 5, 8):
        h = fb.FECHamming(j)
        assert np.array_equal(h.H[:, h.k:], np.eye(j, dtype=int))                 # systematic: the identity on the right
        assert not np.any(h.G.dot(h.H.T) % 2)                                   # G H^T = 0
        assert np.array_equal(h.G[:, :h.k], np.eye(h.k, dtype=int)) and np.array_equal(h.R[:, :h.k], np.eye(h.k, dtype=int)) and not h.R[:, h.k:].any()
        x = np.random.default_rng(j).integers(0, 2, 3 * h.k)
        assert np.array_equal(h.hamm_encoder_host(x), (x.reshape(3, h.k).dot(h.G) % 2).reshape(-1))
    big = fb.FECHamming(12)
    assert big._G is None and big._R is None and big.H.shape == (12, 4095)     # the large matrices are not built unless asked for
    g5 = h.hamm_gen(5)
    assert g5[3:] == (31, 26) and g5[0].shape == (26, 31)


def test_signatures_match_reference(conv):
    for cls in ("FECHamming", "FECCyclic"):
        for name, sig in conv["signatures"][cls].items():
            ours = [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(getattr(getattr(fb, cls), name)).parameters.values()]
            assert ours == sig, (cls, name)
    for name in ("hamm_encoder_host", "hamm_decoder_host"):
        assert inspect.signature(getattr(fb.FECHamming, name)) == inspect.signature(getattr(fb.FECHamming, name[:-5]))
    for name in ("cyclic_encoder_host", "cyclic_decoder_host"):
        assert inspect.signature(getattr(fb.FECCyclic, name)) == inspect.signature(getattr(fb.FECCyclic, name[:-5]))


def test_conventions_are_settled_before_any_device_call(conv, caplog):
    """what the reference raises as ValueError, both forms raise as ValueError (they share the checks, which run before the device is
    touched); the deliberate differences are the ones the fixture names"""
    assert set(conv["deliberate_differences"]) == {"j_range", "bit_values", "containers", "empty", "lazy_matrices", "bounds", "in_place"}
    with caplog.at_level("INFO"):
        ham, cyc = fb.FECHamming(3), fb.FECCyclic('1011')
    assert [r.getMessage() for r in caplog.records] == ["(7,4) hamming code object", "(7,4) cyclic code object"]
    rng = np.random.default_rng(20)
    x4 = rng.integers(0, 2, 8)
    c7 = ham.hamm_encoder_host(x4).astype(int)
    calls = {"hamm_encoder": (ham, x4, 4, np.float64), "hamm_decoder": (ham, c7, 7, np.int64),
             "cyclic_encoder": (cyc, x4, 4, np.int64), "cyclic_decoder": (cyc, c7, 7, np.int64)}
    for name, (obj, good, per, dt) in calls.items():
        ref = conv["methods"][name]
        for f in (getattr(obj, name), getattr(obj, name + "_host")):
            for key, bad in (("float", good.astype(np.float64)), ("bad_length", good[:per + 1]), ("short", good[:per - 1])):
                assert ref[key]["raises"] == "ValueError"
                with pytest.raises(ValueError) as e:
                    f(bad)
                assert str(e.value) == ref[key]["message"], (name, key)
            for bad in (np.where(np.arange(good.size) == 1, 2, good), np.where(np.arange(good.size) == 1, -1, good)):    # deliberate: bit_values
                with pytest.raises(ValueError, match="0 or 1"):
                    f(bad)
            y = f(np.zeros(0, dtype=int))                                                                                # deliberate: empty
            assert y.dtype == dt and y.shape == (0,) and "raises" in ref["empty"]
        host = getattr(obj, name + "_host")
        y = host(good)
        assert list(y.shape) == ref["good"]["shape"] and str(y.dtype) == ref["good"]["dtype"] == np.dtype(dt).name
        for same in (good.astype(np.int32), good.astype(np.uint8), [int(v) for v in good], tuple(int(v) for v in good)):   # deliberate: containers
            assert np.array_equal(host(same), y)
        assert "raises" in ref["int32"] and "raises" in ref["uint8"] and ref["list"]["raises"] == "TypeError"
    kept = c7.copy()
    kept[2] ^= 1
    seen = kept.copy()
    ham.hamm_decoder_host(seen)
    assert np.array_equal(seen, kept)                                                                                    # deliberate: in_place
    assert conv["cyclic_encoder_ignores_G"] and np.array_equal(cyc.cyclic_encoder_host(x4, '1101'), cyc.cyclic_encoder_host(x4))
    # constructors
    with pytest.raises(ValueError, match=conv["hamming_j2"]["message"]):
        fb.FECHamming(2)
    for bad in ('0011', '1010'):
        with pytest.raises(ValueError, match="Invalid generator polynomial"):
            fb.FECCyclic(bad)
    assert conv["cyclic_bad_first"]["raises"] == conv["cyclic_bad_last"]["raises"] == "ValueError" and "raises" not in conv["cyclic_j2"]
    for bad in (lambda: fb.FECHamming(17), lambda: fb.FECCyclic('111'), lambda: fb.FECCyclic('1' + '0' * 16 + '1'), lambda: fb.hamming_tables(2),   # deliberate: j_range
                lambda: fb.cyclic_tables('1021')):
        with pytest.raises(ValueError):
            bad()
    assert fb.FECHamming(16).n == 65535 and fb.FECCyclic('11010000000010001').k == 65519
    assert not hasattr(fb, "ser2ber") and not hasattr(fb, "block_single_error_Pb_bound")
    assert set(conv["ref_bits_per_s"]) == {"ham%d" % j for j in (3, 4, 5, 6, 7, 8, 10)} | {"cyc" + G for G in ('1011', '10011', '101001', '1100001', '10100001', '101110001', '1101') + NONPRIMITIVE}


def test_c_abi_rejects_bad_arguments_without_a_device():
    import ctypes
    L = _ffi.load()
    h = ctypes.c_void_p(0)
    enc, syn, trap = fb.hamming_tables(3)

    def create(n, k, e, s, t):
        ptr = [_ffi._ptr(np.ascontiguousarray(v, dtype=np.uint32)) if v is not None else None for v in (e, s, t)]
        return L.skdsp_blockcode_create(n, k, ptr[0], ptr[1], ptr[2], ctypes.byref(h))
    big = np.zeros(2 ** 17, dtype=np.uint32)
    assert create(2 ** 17 - 1, 2 ** 17 - 18, big, big, big) == -1 and b"65535" in L.skdsp_last_error()       # j = 17
    assert create(3, 1, enc, syn, trap) == -1 and b"3 ... 16" in L.skdsp_last_error()                         # j = 2
    assert create(8, 5, enc, syn, trap) == -1                                                                  # n is not 2^j - 1
    assert create(7, 4, None, syn, trap) == -1 and create(7, 4, enc, None, trap) == -1 and create(7, 4, enc, syn, None) == -1
    assert L.skdsp_blockcode_create(7, 4, _ffi._ptr(enc), _ffi._ptr(syn), _ffi._ptr(trap), None) == -1
    wide = syn.copy()
    wide[5] = 8
    assert create(7, 4, enc, wide, trap) == -1 and b"does not fit" in L.skdsp_last_error()                    # a table word of 4 bits for j = 3
    assert h.value is None
    for name in ("encode", "encode_dev", "decode", "decode_dev"):
        assert getattr(L, "skdsp_blockcode_" + name)(None, None, 1, None) == -1 and b"not a block code handle" in L.skdsp_last_error()


# ---------------------------------------------------------------------------------------------------------------- the kernels' plan on the CPU
def build_emul(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "host", "blockcode_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("blk"), "blockcode_emul", [])


def plan_of(exe, n, k):
    """{form, blocks_per_wg, threads, lds} of blk::plan_make(n, k)"""
    words = subprocess.check_output([exe, str(n), str(k)]).decode().split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def run_emul(exe, tmp, code, mode, bits, in_off=0, out_off=0):
    tab, inp, outp = str(tmp / "tables.u32"), str(tmp / "in.u8"), str(tmp / "out.u8")
    np.concatenate((code._enc, code._syn, code._trap)).astype(np.uint32).tofile(tab)
    np.asarray(bits, dtype=np.uint8).tofile(inp)
    subprocess.check_call([exe, str(code.n), str(code.k), str(mode), tab, inp, outp, str(in_off), str(out_off)], stdout=subprocess.DEVNULL)
    return np.fromfile(outp, dtype=np.uint8)


def test_plan_forms_and_thresholds(emul):
    forms = {j: plan_of(emul, 2 ** j - 1, 2 ** j - 1 - j) for j in range(3, 17)}
    assert [forms[j]["form"] for j in range(3, 17)] == [FORM_LANE] * 4 + [FORM_WAVE] * 6 + [FORM_GROUP] * 4
    for j, p in forms.items():
        assert p["lds"] <= 160 * 1024 and p["lds"] % 16 == 0 and p["threads"] % 64 == 0
        if p["form"] == FORM_WAVE:
            assert p["blocks_per_wg"] % (p["threads"] // 64) == 0
    assert subprocess.call([emul, "131071", "131054"], stderr=subprocess.DEVNULL) == 5 and subprocess.call([emul, "3", "1"], stderr=subprocess.DEVNULL) == 5


def test_kernel_plan_host_emulation_reproduces_the_fixtures(g20, emul, tmp_path):
    """every captured case (lane form: j <= 6; wave form: j = 7, 8, 10) through the kernels' own staging and per-block functions"""
    g, cases = g20
    for c in cases:
        x, ref = bits_of(g, c)
        y = run_emul(emul, tmp_path, code_of(c), 0 if c["fn"] == "encode" else 1, x)
        assert np.array_equal(y, ref), c["key"]


def test_sanitized_emulation_every_form_at_unaligned_windows(tmp_path):
    """-fsanitize=address,undefined on the stand-alone emulation: each plan form, several workgroups with a partial last one, the input and
    output windows 0, 1, 3 and 15 bytes off a 16-byte boundary inside exact-size allocations (a staging overrun shows here, not on a GPU)"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this toolchain cannot link the address / undefined-behaviour sanitizer runtimes")
    exe = build_emul(tmp_path, "blockcode_emul_san", san)
    rng = np.random.default_rng(2021)
    seen = set()
    for code in (fb.FECHamming(3), fb.FECCyclic('1100001'), fb.FECHamming(7), fb.FECCyclic('10100001'), fb.FECHamming(12), fb.FECHamming(13), fb.FECHamming(16)):
        p = plan_of(exe, code.n, code.k)
        seen.add(p["form"])
        nblocks = {FORM_LANE: p["blocks_per_wg"] + 1, FORM_WAVE: p["blocks_per_wg"] + 3, FORM_GROUP: 2}[p["form"]]
        x, c = one_error_words(code, rng, nblocks)
        want_code, want_bits = method(code, "encode", True)(x).astype(np.uint8), method(code, "decode", True)(c).astype(np.uint8)
        for in_off, out_off in ((0, 0), (1, 3), (3, 15), (15, 1)):
            assert np.array_equal(run_emul(exe, tmp_path, code, 0, x, in_off, out_off), want_code), (code.n, in_off, out_off)
            assert np.array_equal(run_emul(exe, tmp_path, code, 1, c, in_off, out_off), want_bits), (code.n, in_off, out_off)
    assert seen == {FORM_LANE, FORM_WAVE, FORM_GROUP}
