"""fec_block.FECHamming / FECCyclic on the MI355X (csrc/blockcode.hip): every case captured from the real reference (g20) bit for bit,
the edges of the three mappings (block counts read from the plan) against the vectorised host restatement (which
tests/test_fecblock_cpu.py pins to the same captures), round trips with a flipped bit at every position, *_dev calls on unaligned
windows of larger device buffers, a many-workgroup case run twice, and the C ABI's argument errors.  Outputs are bits: every comparison
is array_equal, nothing has a tolerance and nothing asserts a time."""
import ctypes

import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, fec_block as fb
from test_fecblock_cpu import (FORM_GROUP, FORM_LANE, FORM_WAVE, bits_of, code_of, emul, g20, method, one_error_words,  # noqa: F401  (fixtures)
                               plan_of)

pytestmark = pytest.mark.gpu


def make(spec):
    return fb.FECHamming(spec) if isinstance(spec, int) else fb.FECCyclic(spec)


def test_every_reference_case_bit_for_bit(g20):
    g, cases = g20
    for c in cases:
        x, ref = bits_of(g, c)
        _ffi.debug_path()
        y = method(code_of(c), c["fn"], False)(x)
        assert _ffi.debug_path() == ["blockcode"], c["key"]
        assert y.dtype == ref.dtype and y.shape == ref.shape, (c["key"], y.dtype, y.shape)
        assert np.array_equal(y, ref), (c["key"], int(np.sum(y != ref)))


@pytest.mark.parametrize("spec,form", [(3, FORM_LANE), (6, FORM_LANE), (7, FORM_WAVE), (10, FORM_WAVE), ('10100001', FORM_WAVE), (13, FORM_GROUP),
                                       (16, FORM_GROUP)])
def test_mapping_edges_equal_the_host_restatement(spec, form, emul):
    """lane per block: a lone block, a wave's last lane and the next wave's first, one block past a workgroup's run; wave per block: fewer
    blocks than waves, exactly one round, a second round, one block past the run; workgroup per block: one block and several"""
    code = make(spec)
    plan = plan_of(emul, code.n, code.k)
    assert plan["form"] == form
    counts = {FORM_LANE: (1, 2, 63, 64, 65, plan["blocks_per_wg"] + 1), FORM_WAVE: (1, 3, 4, 5, plan["blocks_per_wg"] + 1), FORM_GROUP: (1, 3)}[form]
    rng = np.random.default_rng(code.n)
    for nblocks in counts:
        x, c = one_error_words(code, rng, nblocks)
        _ffi.debug_path()
        y_enc = method(code, "encode", False)(x)
        assert _ffi.debug_path() == ["blockcode"]      # (a repeated engine name is noted once: read the path after each call)
        y_dec = method(code, "decode", False)(c)
        assert _ffi.debug_path() == ["blockcode"]
        ref_enc, ref_dec = method(code, "encode", True)(x), method(code, "decode", True)(c)
        assert y_enc.dtype == ref_enc.dtype and np.array_equal(y_enc, ref_enc), (spec, nblocks, "encode")
        assert y_dec.dtype == ref_dec.dtype and np.array_equal(y_dec, ref_dec), (spec, nblocks, "decode")


@pytest.mark.parametrize("spec", [3, 7, 10, '1011', '10100001', 13])
def test_round_trip(spec):
    code = make(spec)
    x = np.random.default_rng(7).integers(0, 2, 5 * code.k)
    assert np.array_equal(method(code, "decode", False)(method(code, "encode", False)(x).astype(np.int64)), x)


@pytest.mark.parametrize("j", [3, 7, 10])
def test_round_trip_with_one_flipped_bit_at_every_position(j):
    code = fb.FECHamming(j)
    x = np.random.default_rng(j).integers(0, 2, code.k)
    word = code.hamm_encoder(x).astype(np.int64)
    c = np.tile(word, (code.n, 1))
    c[np.arange(code.n), np.arange(code.n)] ^= 1            # block i: position i flipped
    assert np.array_equal(code.hamm_decoder(c.reshape(-1)), np.tile(x, code.n))


@pytest.mark.parametrize("spec", [6, '10100001', 13])
def test_device_windows_at_unaligned_offsets(spec, emul):
    """the windows sit 1, 3 and 15 bytes into larger device buffers; around the input lie 0xFF bytes (no bit value: read as a bit they would
    change a result), around the output a guard pattern that must come back untouched"""
    code = make(spec)
    plan = plan_of(emul, code.n, code.k)
    nblocks = plan["blocks_per_wg"] + 2 if plan["form"] != FORM_GROUP else 2
    x, c = one_error_words(code, np.random.default_rng(31), nblocks)
    kern = code._kernel()
    pad = 64
    for fn, inp, ref in ((kern.encode_dev, x, method(code, "encode", True)(x)), (kern.decode_dev, c, method(code, "decode", True)(c))):
        ref = ref.astype(np.uint8)
        for in_off, out_off in ((1, 3), (3, 15), (15, 1)):
            din, dout = _ffi.DeviceBytes(inp.size + 2 * pad), _ffi.DeviceBytes(ref.size + 2 * pad)
            host_in = np.full(din.nbytes, 0xFF, dtype=np.uint8)
            host_in[pad + in_off:pad + in_off + inp.size] = inp
            din.write(host_in)
            guard = ((np.arange(dout.nbytes) * 37 + 11) % 251 + 2).astype(np.uint8)      # never 0 / 1
            dout.write(guard)
            _ffi.debug_path()
            fn(din.ptr + pad + in_off, nblocks, dout.ptr + pad + out_off)
            assert _ffi.debug_path() == ["blockcode"]
            got = dout.read()
            lo, hi = pad + out_off, pad + out_off + ref.size
            assert np.array_equal(got[lo:hi], ref), (spec, fn.__name__, in_off, out_off)
            assert np.array_equal(got[:lo], guard[:lo]) and np.array_equal(got[hi:], guard[hi:]), (spec, fn.__name__, in_off, out_off)
            din.free()
            dout.free()


def test_many_workgroups_twice_and_against_the_host():
    code = fb.FECHamming(7)
    nblocks = 2 ** 17
    rng = np.random.default_rng(17)
    c = rng.integers(0, 2, (nblocks, code.n), dtype=np.uint8)
    kern = code._kernel()
    first, second = kern.decode(c), kern.decode(c)
    assert np.array_equal(first, second)
    assert np.array_equal(first.reshape(-1), code.hamm_decoder_host(c.reshape(-1)))


def test_c_abi_argument_errors_come_back_without_a_launch():
    L = _ffi.load()
    h = ctypes.c_void_p(0)
    enc, syn, trap = fb.hamming_tables(3)
    big = np.zeros(2 ** 17, dtype=np.uint32)
    _ffi.debug_path()
    assert L.skdsp_blockcode_create(2 ** 17 - 1, 2 ** 17 - 18, _ffi._ptr(big), _ffi._ptr(big), _ffi._ptr(big), ctypes.byref(h)) == -1      # j = 17
    wide = syn.copy()
    wide[0] = 9
    assert L.skdsp_blockcode_create(7, 4, _ffi._ptr(enc), _ffi._ptr(wide), _ffi._ptr(trap), ctypes.byref(h)) == -1                          # a word too wide
    assert L.skdsp_blockcode_create(7, 4, None, _ffi._ptr(syn), _ffi._ptr(trap), ctypes.byref(h)) == -1 and h.value is None
    from sk_dsp_comm_amd import fec_conv
    vit = fec_conv.FECConv(('111', '101'), 10)._kernel()                                                                                    # a handle of the wrong kind
    kern = fb.FECHamming(3)._kernel()
    buf = _ffi.DeviceBytes(64)
    for name in ("encode_dev", "decode_dev"):
        fn = getattr(L, "skdsp_blockcode_" + name)
        assert fn(ctypes.c_void_p(vit.h), ctypes.c_void_p(buf.ptr), 1, ctypes.c_void_p(buf.ptr + 32)) == -1 and b"not a block code handle" in L.skdsp_last_error()
        assert fn(ctypes.c_void_p(kern.h), None, 1, ctypes.c_void_p(buf.ptr)) == -1 and fn(ctypes.c_void_p(kern.h), ctypes.c_void_p(buf.ptr), 1, None) == -1
        assert fn(ctypes.c_void_p(kern.h), ctypes.c_void_p(buf.ptr), -1, ctypes.c_void_p(buf.ptr + 32)) == -1
        assert fn(ctypes.c_void_p(kern.h), None, 0, None) == 0                                                                              # no blocks: a no-op
    host = np.zeros(7, dtype=np.uint8)
    assert L.skdsp_blockcode_decode(ctypes.c_void_p(vit.h), _ffi._ptr(host), 1, _ffi._ptr(host)) == -1
    assert L.skdsp_blockcode_decode(ctypes.c_void_p(kern.h), None, 1, _ffi._ptr(host)) == -1
    assert _ffi.debug_path() == []


@pytest.mark.parametrize("nblocks", [1, 37])
def test_host_forms_equal_the_device_forms_bit_for_bit(nblocks):
    """skdsp_blockcode_encode / _decode (host pointers) against their _dev forms on the same bits, one error in every other code word"""
    rng = np.random.default_rng(62 + nblocks)
    for code in (fb.FECHamming(3), fb.FECCyclic('10011')):
        k = code._kernel()
        bits = rng.integers(0, 2, (nblocks, k.k), dtype=np.uint8)
        cw = k.encode(bits)
        din, dout = _ffi.DeviceBytes(bits.size), _ffi.DeviceBytes(cw.size)
        din.write(bits.reshape(-1))
        k.encode_dev(din.ptr, nblocks, dout.ptr)
        assert np.array_equal(dout.read(), cw.reshape(-1))
        cw[::2, rng.integers(0, k.n)] ^= 1
        back = k.decode(cw)
        dout.write(cw.reshape(-1))
        k.decode_dev(dout.ptr, nblocks, din.ptr)
        assert np.array_equal(back, bits) and np.array_equal(din.read(), back.reshape(-1))
