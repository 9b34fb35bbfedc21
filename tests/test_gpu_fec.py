"""fec_conv.FECConv.viterbi_decoder / viterbi_decoder_rows on the MI355X (csrc/viterbi.hip): every case captured from the real
reference (g19) bit for bit, the carried decoder state, the rows form at the wave layouts' edges against the float64 host
restatement (which tests/test_fec_cpu.py pins to the same captures), determinism and the argument errors.  Outputs are 0. / 1.:
every comparison is array_equal, nothing has a tolerance and nothing asserts a time."""
import numpy as np
import pytest

from sk_dsp_comm_amd import _ffi, fec_conv as fc
from test_fec_cpu import g19, received  # noqa: F401  (g19: module-scoped fixture)

pytestmark = pytest.mark.gpu

HALF = {3: ('111', '101'), 5: ('11101', '10011'), 7: ('1111001', '1011011'), 9: ('111101011', '101110001')}


def noisy(cc, rng, nrow, nsym, q=3, sigma=0.9):
    """nrow different noisy code words as soft values (fractions, some below 0 and above the top level)"""
    K = cc.constraint_length
    rows = [cc.conv_encoder(rng.integers(0, 2, nsym), '0' * (K - 1))[0] for _ in range(nrow)]
    return ((2 * np.array(rows) - 1) + sigma * rng.standard_normal((nrow, nsym * len(cc.G_polys))) + 1) / 2 * (2 ** q - 1)


def test_every_reference_case_bit_for_bit(g19):
    g, cases, _ = g19
    for c in cases:
        cc = fc.FECConv(tuple(c["G"]), c["depth"])
        for i in range(c["calls"]):       # calls of one case share the object: the carried state is part of what is compared
            _ffi.debug_path()
            y = cc.viterbi_decoder(received(g["%s_x%d" % (c["key"], i)]), c["metric"], c["quant_level"])
            assert _ffi.debug_path() == ["viterbi"], c["key"]
            ref = g["%s_y%d" % (c["key"], i)]
            assert y.dtype == np.float64 and y.shape == ref.shape, (c["key"], i, y.shape, ref.shape)
            assert np.array_equal(y, ref), (c["key"], i, int(np.sum(y != ref)))


def test_state_carry_and_reset(g19):
    g, cases, _ = g19
    for key in ("carry_soft_h3", "carry_soft_h7", "carry_soft_t5", "carry_soft_h9", "carry_unq_h7", "carry_hard_h7"):
        c = next(c for c in cases if c["key"] == key)
        xs = [received(g["%s_x%d" % (key, i)]) for i in range(3)]
        ref = [g["%s_y%d" % (key, i)] for i in range(3)]
        cc = fc.FECConv(tuple(c["G"]), c["depth"])
        for i in range(3):
            assert np.array_equal(cc.viterbi_decoder(xs[i], c["metric"], c["quant_level"]), ref[i]), (key, i)
        assert ref[1].size == 0                                           # too short to emit, yet call 3 saw its symbols
        host = fc.FECConv(tuple(c["G"]), c["depth"])
        for i in range(3):
            host.viterbi_decoder_host(xs[i], c["metric"], c["quant_level"])
        cc.viterbi_decoder_rows(np.stack((xs[2], xs[2][::-1])), c["metric"], c["quant_level"])    # the rows form neither reads nor writes the state:
        assert np.array_equal(cc.viterbi_decoder(xs[0], c["metric"], c["quant_level"]),           # a fourth call continues the third
                              host.viterbi_decoder_host(xs[0], c["metric"], c["quant_level"])), key
        cc.reset()
        assert np.array_equal(cc.viterbi_decoder(xs[0], c["metric"], c["quant_level"]), ref[0]), key
    # the carried metrics of one family are not the other's
    with pytest.raises(ValueError, match="reset"):
        cc.viterbi_decoder(xs[0].astype(np.float64), 'unquant')
    cc.reset()
    cc.viterbi_decoder(xs[0].astype(np.float64), 'unquant')


@pytest.mark.parametrize("K,nrows", [(3, (1, 2, 15, 16, 17)), (7, (1, 3)), (9, (2,))])
def test_rows_equal_the_host_restatement(K, nrows):
    """K = 3: 16 streams per wave, partial and just-overflowing wave; K = 7: one state per lane; K = 9: four states per lane"""
    rng = np.random.default_rng(100 + K)
    cc = fc.FECConv(HALF[K], 5 * K)
    for nrow in nrows:
        x = noisy(cc, rng, nrow, 5 * K + 150 + nrow)
        _ffi.debug_path()
        y = cc.viterbi_decoder_rows(x)
        assert _ffi.debug_path() == ["viterbi"]
        assert y.dtype == np.float64 and y.shape == (nrow, 151 + nrow)
        for r in range(nrow):
            assert np.array_equal(y[r], cc.viterbi_decoder_host(x[r], carry=False)), (K, nrow, r)


def test_rows_all_metrics_and_rate_third():
    rng = np.random.default_rng(7)
    cc = fc.FECConv(('11111', '11011', '10101'), 70)     # four-word histories
    x = noisy(cc, rng, 9, 200, q=1, sigma=1.2)
    assert np.array_equal(cc.viterbi_decoder_rows(x / 1.0, 'unquant'), cc.viterbi_decoder_rows_host(x, 'unquant'))
    assert np.array_equal(cc.viterbi_decoder_rows(x * 63, 'soft', 6), cc.viterbi_decoder_rows_host(x * 63, 'soft', 6))
    xb = (x[:, :599] > 0.5).astype(np.int64)              # 599 values: a short last symbol
    y = cc.viterbi_decoder_rows(xb, 'hard')
    assert y.shape == (9, 200 - 69) and np.array_equal(y, cc.viterbi_decoder_rows_host(xb, 'hard'))


def test_rows_many_workgroups():
    """K = 5, 513 rows of 4096 symbols: 129 waves of four streams, the last one with a single row"""
    rng = np.random.default_rng(55)
    cc = fc.FECConv(HALF[5], 25)
    x = noisy(cc, rng, 513, 4096)
    y = cc.viterbi_decoder_rows(x)
    assert y.shape == (513, 4096 - 24)
    assert np.array_equal(y, cc.viterbi_decoder_rows_host(x))
    for r in (0, 255, 512):
        assert np.array_equal(y[r], cc.viterbi_decoder_host(x[r], carry=False)), r


def test_rows_ties_beside_noise():
    """two waves' worth of rows, all-zero hard rows (every comparison a tie, every metric the minimum) between noisy ones: a
    minimum, ballot or find-first that leaks across the streams of a wave would move the noisy rows' bits or the tied rows'"""
    rng = np.random.default_rng(3)
    for K in (3, 5):
        cc = fc.FECConv(HALF[K], 5 * K)
        nrow = 2 * (64 // cc.Nstates)
        x = (noisy(cc, rng, nrow, 300, q=1, sigma=1.0) > 0.5).astype(np.int64)
        x[1::3] = 0
        x[nrow - 1] = 0
        y = cc.viterbi_decoder_rows(x, 'hard')
        assert np.array_equal(y, cc.viterbi_decoder_rows_host(x, 'hard')), K
        assert not np.any(y[1]) and np.any(y[0])


def test_soft_metrics_at_the_limits_of_the_int32_headroom():
    """|int(x)| = 4095 against quant_level 12 (levels 0 and 4095): the largest branch metrics the 32-bit normalised metrics must hold,
    K = 9 (the longest path from the minimum state) and rate 1/3; the float64 restatement has no such limit"""
    rng = np.random.default_rng(12)
    for G, D in ((HALF[9], 45), (('11110111', '11011001', '10010101'), 40)):
        cc = fc.FECConv(G, D)
        x = rng.choice([-4095.9, -4095.0, 0.0, 4095.0, 4095.9], size=(6, 300 * len(G)))
        x[0] = np.where(np.arange(x.shape[1]) % 2, 4095.0, -4095.0)      # every branch far from both levels or on one of them
        x[1] = -4095.0
        assert np.array_equal(cc.viterbi_decoder_rows(x, 'soft', 12), cc.viterbi_decoder_rows_host(x, 'soft', 12)), G
        assert np.array_equal(cc.viterbi_decoder(x[2], 'soft', 12), cc.viterbi_decoder_host(x[2], 'soft', 12, carry=False)), G
        with pytest.raises(ValueError, match="4095"):
            cc.viterbi_decoder_rows(np.where(x == 0.0, 4096.0, x), 'soft', 12)


def test_long_single_stream():
    """K = 7, rate 1/2, soft, Depth 35, 2^16 symbols: the stateful call, the host restatement and a 1-row rows call agree"""
    rng = np.random.default_rng(35)
    cc = fc.FECConv(HALF[7], 35)
    x = noisy(cc, rng, 1, 1 << 16, sigma=1.0)[0]
    ref = cc.viterbi_decoder_host(x, carry=False)
    y = cc.viterbi_decoder(x)
    assert y.shape == ((1 << 16) - 34,) and np.array_equal(y, ref)
    assert np.array_equal(cc.viterbi_decoder_rows(x[None])[0], ref)


def test_determinism():
    rng = np.random.default_rng(9)
    cc = fc.FECConv(HALF[9], 45)
    x = noisy(cc, rng, 1, 3000, sigma=1.1)[0]
    k = cc._kernel()
    xi = np.trunc(x).astype(np.int16)
    a = k.decode(xi, k.SOFT, 3).tobytes()
    cc.reset()
    assert k.decode(xi, k.SOFT, 3).tobytes() == a
    r = k.decode_rows(np.tile(xi, (5, 1)), k.SOFT, 3)
    assert all(r[i].tobytes() == a for i in range(5))


def test_errors_raise_without_a_launch():
    _ffi.debug_path()
    with pytest.raises(ValueError, match="128"):
        fc.FECConv(HALF[7], 129)
    with pytest.raises(ValueError, match="128"):
        _ffi.ViterbiKernel(HALF[7], 129)
    with pytest.raises(ValueError, match="3 ... 9"):
        fc.FECConv(('1111010111', '1011100011'), 10)
    with pytest.raises(ValueError, match="3 ... 9"):
        _ffi.ViterbiKernel(('1111010111', '1011100011'), 10)
    cc = fc.FECConv(HALF[7], 35)
    x = np.full(200, 3.0)
    for bad in (np.nan, np.inf):
        x[17] = bad
        with pytest.raises(ValueError, match="non-finite"):
            cc.viterbi_decoder(x)
        with pytest.raises(ValueError, match="non-finite"):
            cc.viterbi_decoder_rows(x.reshape(2, 100))
    k = cc._kernel()
    with pytest.raises(ValueError):
        k.decode(np.zeros(201, np.int16), k.SOFT, 3)          # no whole number of symbols
    with pytest.raises(ValueError):
        k.decode(np.zeros(200, np.int16), k.SOFT, 13)
    assert _ffi.debug_path() == []


def test_host_forms_equal_the_device_forms_bit_for_bit():
    """skdsp_viterbi_decode[_rows] (host pointers) against skdsp_viterbi_decode[_rows]_dev on the same values: rows calls at 1 and 3 rows, and the
    stateful call over three pieces -- the middle one shorter than the decision depth, so it returns no bit and only advances the state."""
    rng = np.random.default_rng(61)
    cc = fc.FECConv(HALF[5], 12)
    for nrow, nsym in ((1, 40), (3, 75)):
        x = np.trunc(noisy(cc, rng, nrow, nsym)).astype(np.int16)
        k = _ffi.ViterbiKernel(HALF[5], 12)
        y = k.decode_rows(x, k.SOFT, 3)
        xd, yd = _ffi.DeviceBytes(x.nbytes), _ffi.DeviceBytes(max(y.size, 1))
        xd.write(x.reshape(-1).view(np.uint8))
        k.decode_rows_dev(xd.ptr, x.shape[1], nrow, k.SOFT, 3, yd.ptr)
        assert y.shape == (nrow, k.out_len(x.shape[1])) and y.size and np.array_equal(yd.read(0, y.size), y.reshape(-1)), (nrow, nsym)
    x = np.trunc(noisy(cc, rng, 1, 90)[0]).astype(np.int16)
    kh, kd = _ffi.ViterbiKernel(HALF[5], 12), _ffi.ViterbiKernel(HALF[5], 12)
    sizes = []
    for piece in (x[:80], x[80:84], x[84:]):
        y = kh.decode(piece, kh.SOFT, 3)
        xd, yd = _ffi.DeviceBytes(piece.nbytes), _ffi.DeviceBytes(max(y.size, 1))
        xd.write(piece.view(np.uint8))
        kd.decode_dev(xd.ptr, piece.size, kd.SOFT, 3, yd.ptr)
        assert np.array_equal(yd.read(0, y.size), y), piece.size
        sizes.append(y.size)
    assert sizes[0] > 0 and sizes[2] > 0
